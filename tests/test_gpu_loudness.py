"""GPU: the loudness unit (csrc/loudness.hip) against tests/loudness_ref.py: the K-weighted hop sums and
the gates in float64, the fused true-peak meter against the project's own resampler, the look-ahead limiter against
its float64 restatement, loudness_normalize, and transfer_recording's loudness= argument."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R         # noqa: E402
import loudness_ref as LR     # noqa: E402
import resample_ref as RR     # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                # half an ulp of an fp32 value below 1
CEIL = 10.0 ** (-1.0 / 20.0)
# Largest |device - float64| measured on an MI355X over the limiter cases below (noise of sigma 0.2 with impulses of up
# to 2.0, ceiling -1 dB, look-ahead 110): gain 4.44e-7, y 4.15e-7, against the derived bounds of 3.54e-5 / 7.10e-5.
LIMIT_MEASURED = {"gain": 4.44e-7, "y": 4.15e-7}


@pytest.fixture(scope="module")
def A():
    from ldm_amd import audio
    return audio


@pytest.fixture(scope="module")
def ops():
    from ldm_amd import ops
    return ops


def dev(a, cuda, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(cuda)


def f32(a):
    return np.asarray(a, dtype=np.float32)


# ---- 1. hop sums ------------------------------------------------------------------------------------------------
def hop_inputs(L, seed):
    """noise, a DC step (the high-pass's slow tail crosses many chunks) and all zeros: [3, L] fp32."""
    rng = np.random.default_rng(seed)
    step = np.zeros(L)
    step[L // 3:] = 0.5
    return f32(np.stack([0.3 * rng.standard_normal(L), step, np.zeros(L)]))


@pytest.mark.parametrize("sr", [22050, 48000])
def test_hop_sums_match_float64(A, ops, cuda, sr):
    """Both sides are float64 and differ in operation order only; the poles (radius 0.989 at 22050 Hz) amplify rounding
    by about 1e2: 1e-9 of the row's largest hop sum leaves three orders of margin."""
    hop = A.loudness_hop(sr)
    chunk = ops.loudness_chunk(hop)
    assert chunk >= 1
    sos = A.k_weighting(sr).reshape(-1)
    worst = 0.0
    for n, L in enumerate(sorted({hop - 1, hop, 4 * hop, 4 * hop + 1, chunk - 1, chunk, chunk + 1, 3 * chunk + 17, 44100})):
        x = hop_inputs(L, 40 + n)
        xd = dev(x, cuda)
        got = ops.loudness_hop_sums(xd, hop, sos)
        want = LR.hop_sums(x, sr)
        assert got.dtype == torch.float64 and tuple(got.shape) == want.shape == (3, L // hop)
        if L < hop:
            continue
        g = got.cpu().numpy()
        scale = np.maximum(want.max(axis=1, keepdims=True), 1e-300)
        err = float((np.abs(g - want) / scale).max())
        worst = max(worst, err)
        assert err <= 1e-9, (sr, L, err)
        assert (g[2] == 0.0).all()
        assert torch.equal(got, ops.loudness_hop_sums(xd, hop, sos))                    # repeatable, bitwise
        for b in range(3):                                                              # and independent of B
            assert torch.equal(got[b:b + 1], ops.loudness_hop_sums(xd[b:b + 1], hop, sos)), (sr, L, b)
    print(f"hop sums at {sr} Hz: largest difference {worst:.2e} of the row's largest hop sum")


# ---- 2. the gates -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [22050, 48000])
def test_gates_match_the_reference(A, cuda, sr):
    x = f32(LR.gated_signal(sr))
    assert x.size <= 2 * sr
    want, l = LR.gate(LR.hop_sums(x, sr), sr)
    assert LR.threshold_margin(l, want[2]) >= 0.1                 # no block within 0.1 LU of either threshold
    assert 0 < want[1] < int((l > -70.0).sum()) < want[3]         # both gates remove blocks
    rows = np.stack([x, np.zeros_like(x), 0.5 * x])
    got = A.loudness_stats(dev(rows, cuda), sr).cpu().numpy()
    assert got.shape == (3, 4)
    assert abs(got[0, 0] - want[0]) <= 1e-9 and got[0, 1] == want[1] and got[0, 3] == want[3]
    assert abs(got[0, 2] - want[2]) <= 1e-9
    assert got[1, 0] == -np.inf and got[1, 1] == 0 and got[1, 2] == -np.inf and got[1, 3] == want[3]
    assert abs(got[2, 0] - (want[0] + 20.0 * np.log10(0.5))) <= 1e-6 and got[2, 1] == want[1]
    one = A.loudness_stats(dev(x, cuda), sr)
    assert tuple(one.shape) == (4,) and torch.equal(one, A.loudness_stats(dev(rows, cuda), sr)[0])
    hop = A.loudness_hop(sr)
    for L in (4 * hop - 1, hop - 1, 1):                            # shorter than one block
        s = A.loudness_stats(dev(x[:L], cuda), sr).cpu().numpy()
        assert s[0] == -np.inf and s[1] == 0 and s[3] == 0
    il = A.integrated_loudness(dev(rows, cuda), sr)
    assert il.dtype == torch.float64 and tuple(il.shape) == (3,) and il.is_cuda


def test_full_scale_sine_reads_what_the_reference_reads(A, cuda):
    for sr in (48000, 22050):
        x = f32(LR.sine(997.0, 2.0, sr))
        got, want = float(A.integrated_loudness(dev(x, cuda), sr)), LR.integrated_loudness(x, sr)
        print(f"997 Hz full scale, 2 s at {sr} Hz: device {got:.6f} LUFS, reference {want:.6f}")
        assert abs(got - want) <= 1e-9
        assert abs(got + (3.01 if sr == 48000 else 2.981)) <= 0.01


# ---- 3. true peak -----------------------------------------------------------------------------------------------
def test_true_peak(A, cuda):
    """Against the project's own 4x resampler: the same 69-tap sums, so 70 fp32 roundings of sums bounded by
    sum|h| max|y| (the largest phase's sum|h| is 2.31) cover any difference in order."""
    sr = 22050
    up, down, W, table = RR.taps(sr, 4 * sr)
    assert (up, down, W) == (4, 1, 34)
    S = float(np.abs(table).sum(axis=1).max())
    assert S <= 2.31
    rng = np.random.default_rng(9)
    for L in (1, 33, 2047, 2048, 2049, 44100):
        y = f32(0.4 * rng.standard_normal((2, L)))
        y[1] *= 0.01
        yd = dev(y, cuda)
        got = A.true_peak(yd, sr)
        up4 = A.resample(yd, sr, 4 * sr)
        want = torch.maximum(yd.abs().amax(dim=1), up4.abs().amax(dim=1))
        tol = 70 * U * 2.31 * np.abs(y).max(axis=1)
        assert got.dtype == torch.float32 and tuple(got.shape) == (2,)
        assert ((got - want).abs().cpu().numpy() <= tol).all(), (L, got, want)
        assert torch.equal(got, A.true_peak(yd, sr))                                    # bitwise repeatable
        assert torch.equal(got[1], A.true_peak(yd[1], sr))                              # a row alone
    Aamp = 0.8
    x = f32(LR.intersample_sine(sr, Aamp))
    tp = float(A.true_peak(dev(x, cuda), sr))
    print(f"sr/4 sine: sample peak {np.abs(x).max():.6f}, true peak {tp:.6f} (A = {Aamp})")
    assert abs(np.abs(x).max() - Aamp / np.sqrt(2.0)) <= 1e-6
    assert abs(20.0 * np.log10(tp / Aamp)) <= 1e-4 + 20.0 * np.log10(1.0 + 70 * U * 2.31)


# ---- 4. the limiter ---------------------------------------------------------------------------------------------
def limiter_signal(L, tile, seed):
    rng = np.random.default_rng(seed)
    x = 0.2 * rng.standard_normal(L)
    for k, pos in enumerate((0, 2, tile - 1, tile, tile + 1, L - 1)):
        if 0 <= pos < L:
            x[pos] = (2.0 - 0.1 * k) * (-1.0) ** k
    return f32(x)


def limiter_tolerances(x, Lh, sr=22050):
    """The bound on |device - float64| of the gain and of y, with u = 2^-24, X = max|x|, S the largest phase's sum|h|:
      p     69 fma roundings, the sum's own and the fp32 tap table: 71 u S X absolute;
      r     = c / p where p > c: |dr| <= r dp / p + u r <= dp / c + u, and the fp32 ceiling adds u: E_r = 71 u S X / c + 2 u;
      m     a minimum of r's: E_r;
      g     = 1 - sum of 2 Lh + 1 products w_j (1 - m): the subtraction u, each weight 2 u (a sum of weights is 1), the
            fma chain u per step on partial sums below 1, the final subtraction u: E_g = E_r + (2 Lh + 5) u;
      y     = g x: (E_g + u) X."""
    S = float(np.abs(RR.taps(sr, 4 * sr)[3]).sum(axis=1).max())
    X = float(np.abs(x).max())
    e_g = (71.0 * S * X / CEIL + 2.0 + 2 * Lh + 5.0) * U
    return e_g, (e_g + U) * X


def test_limiter_matches_float64(A, ops, cuda):
    sr, Lh = 22050, A.limiter_lookahead(5.0, 22050)
    tile = ops.limit_tile()
    assert Lh == 110 and tile >= 4 * Lh
    worst = {"gain": 0.0, "y": 0.0}
    for n, L in enumerate((tile + Lh, 1, Lh - 1, 2 * Lh + 1, 2 * tile + 3)):
        x = limiter_signal(L, tile, 70 + n)
        up, _, W, taps = A._taps_device(sr, 4 * sr, cuda)
        y, g, mn = ops.limit(dev(x, cuda).unsqueeze(0), taps, up, W, Lh, CEIL, return_gain=True, return_min=True)
        wy, wg = LR.limit(x, sr, CEIL, Lh)
        tol_g, tol_y = limiter_tolerances(x, Lh)
        eg = float(np.abs(g[0].cpu().numpy() - wg).max())
        ey = float(np.abs(y[0].cpu().numpy() - wy).max())
        print(f"limiter L {L}: gain err {eg:.2e} (bound {tol_g:.2e}), y err {ey:.2e} (bound {tol_y:.2e}), "
              f"deepest gain {wg.min():.4f}")
        assert eg <= tol_g and ey <= tol_y, (L, eg, ey)
        assert wg.min() < 0.6 and float(mn[0]) == float(g.min())
        worst["gain"], worst["y"] = max(worst["gain"], eg), max(worst["y"], ey)
        y2, g2 = A.limit(dev(x, cuda), return_gain=True)                               # the public form, with its trim
        assert torch.equal(g2, g[0]) and tuple(y2.shape) == (L,)
    print(f"limiter: largest differences {worst} (recorded {LIMIT_MEASURED})")


def test_limiter_leaves_a_quiet_signal_alone(A, cuda):
    rng = np.random.default_rng(12)
    x = dev(f32(0.1 * rng.standard_normal((2, 9000))), cuda)
    assert float(A.true_peak(x).max()) < CEIL
    y, g = A.limit(x, return_gain=True)
    assert torch.equal(y, x) and bool((g == 1.0).all())
    assert torch.equal(A.limit(x[0]), x[0])


@pytest.mark.parametrize("lookahead_ms", [5.0, 0.0, 20.0])
def test_limit_holds_the_ceiling(A, ops, cuda, lookahead_ms):
    tile = ops.limit_tile()
    x = np.stack([limiter_signal(tile + 300, tile, 81), 3.0 * limiter_signal(tile + 300, tile, 82),
                  0.05 * limiter_signal(tile + 300, tile, 83)])
    xd = dev(x, cuda)
    out = A.limit(xd, ceiling_db=-1.0, lookahead_ms=lookahead_ms)
    tp = A.true_peak(out).cpu().numpy()
    print(f"limit, look-ahead {lookahead_ms} ms: true peaks {tp} (ceiling {CEIL:.6f})")
    assert float(out.abs().max()) <= CEIL
    assert (tp <= CEIL * (1.0 + 2.0 ** -22)).all()
    assert (tp[:2] >= CEIL * 0.99).all()                          # limited, not crushed
    assert torch.equal(out[2], xd[2])                             # the quiet row is untouched
    if lookahead_ms == 0.0:                                        # Lh = 0: a pure per-sample gain
        y, g = A.limit(xd[0], lookahead_ms=0.0, return_gain=True)
        r = np.minimum(1.0, CEIL / LR.envelope(x[0], 22050))
        assert np.abs(g.cpu().numpy() - r).max() <= limiter_tolerances(x[0], 0)[0]


def test_lookahead_over_the_cap_raises(A, ops, cuda):
    from ldm_amd import _lib as L
    x = torch.zeros((1, 4096), device=cuda)
    with pytest.raises(ValueError, match="fit"):
        A.limit(x, lookahead_ms=80.0)                              # 1764 samples
    up, _, W, taps = A._taps_device(22050, 88200, cuda)
    with pytest.raises(ValueError, match="look-ahead"):
        ops.limit(x, taps, up, W, ops.LIMIT_MAX_LOOKAHEAD + 1, CEIL)
    y = torch.empty_like(x)
    with pytest.raises(L.LDMError, match="lookahead"):
        L.call("ldm_limit", x.data_ptr(), 1, 4096, taps.data_ptr(), 4, W, ops.LIMIT_MAX_LOOKAHEAD + 1, CEIL,
               y.data_ptr(), None, None, None, ops.stream_handle())
    out, _, _ = ops.limit(x, taps, up, W, ops.LIMIT_MAX_LOOKAHEAD, CEIL)               # the cap itself runs
    assert torch.equal(out, x)


# ---- 5. loudness_normalize --------------------------------------------------------------------------------------
def test_loudness_normalize(A, cuda):
    sr = 22050
    rng = np.random.default_rng(15)
    x = LR.sine(440.0, 2.0, sr) + 0.3 * rng.standard_normal(2 * sr)
    x = f32(x * 10.0 ** ((-30.0 - LR.integrated_loudness(x, sr)) / 20.0))              # -30 LUFS
    rows = dev(np.stack([x, np.zeros_like(x)]), cuda)
    out, info = A.loudness_normalize(rows, -23.0)
    print(f"loudness_normalize: {info}")
    assert set(info) == set(A.LOUDNESS_INFO_KEYS) and all(len(v) == 2 for v in info.values())
    assert abs(info["input_lufs"][0] + 30.0) <= 0.01 and abs(info["gain_db"][0] - 7.0) <= 0.01
    assert info["max_reduction_db"][0] == 0 and info["max_reduction_db"][1] == 0       # the limiter did not engage
    assert abs(info["output_lufs"][0] + 23.0) <= 0.05
    assert abs(float(A.integrated_loudness(out[0])) + 23.0) <= 0.05
    assert info["input_lufs"][1] == -np.inf and info["gain_db"][1] == 0 and info["output_lufs"][1] == -np.inf
    assert torch.equal(out[1], rows[1])                                                # a -inf row comes back unchanged
    assert info["true_peak_db"][0] <= -1.0
    loud, info2 = A.loudness_normalize(rows[0], -3.0)                                  # now the limiter has to work
    assert tuple(loud.shape) == (2 * sr,) and isinstance(info2["gain_db"], float)
    assert info2["max_reduction_db"] > 0 and info2["true_peak_db"] <= -1.0 + 1e-4
    assert info2["output_lufs"] <= -3.0 + 0.05
    assert float(A.true_peak(loud)) <= CEIL * (1.0 + 2.0 ** -22)


def test_normalize_audio_keeps_the_callers_type(A, cuda):
    from data.audio_processor import AudioPreprocessor
    ap = AudioPreprocessor()
    x = f32(0.05 * LR.sine(440.0, 1.0, 22050))
    a = ap.normalize_audio(x)
    assert isinstance(a, np.ndarray) and a.dtype == np.float32 and a.shape == x.shape
    t = ap.normalize_audio(dev(x, cuda), target_lufs=-20.0, true_peak_db=-2.0)
    assert torch.is_tensor(t) and t.is_cuda and tuple(t.shape) == x.shape
    assert abs(float(A.integrated_loudness(dev(a, cuda))) + 23.0) <= 0.05
    assert abs(float(A.integrated_loudness(t)) + 20.0) <= 0.05


# ---- 6. transfer_recording --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transfer(cuda):
    import models.model as M
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    model = M.LDM(32, pretrained_path="").eval().to(cuda)
    frames, overlap, T_total = 128, 32, 224                                 # two windows: [0, 128) and [96, 224)
    L = (T_total - 1) * HOP
    content = dev(R.test_signal(L).astype(np.float32), cuda)
    style = dev(R.test_signal(150 * HOP, variant=1), cuda)
    kw = dict(frames=frames, overlap=overlap, num_timesteps=2, n_iter=2, nnls_iters=2, seed=4)

    def run(**extra):
        return transfer_recording(model, content, style, **dict(kw, **extra))
    return run, content


def test_transfer_without_loudness_is_the_call_it_was(transfer):
    run, _ = transfer
    a, b = run(solver="dpmpp2m", loudness=None), run(solver="dpmpp2m")
    assert torch.equal(a.audio, b.audio) and torch.equal(a.mel_power, b.mel_power)
    assert not hasattr(a, "loudness")


@pytest.mark.parametrize("vocoder", ["griffinlim", "content"])
def test_transfer_matches_the_contents_loudness(A, transfer, vocoder):
    run, content = transfer
    res = run(solver="dpmpp2m", vocoder=vocoder, loudness="content", report=True)
    info = res.loudness
    print(f"transfer ({vocoder}): {info}")
    assert set(info) == set(A.LOUDNESS_INFO_KEYS) | {"content_lufs"}
    want = float(A.integrated_loudness(content))
    got = float(A.integrated_loudness(res.audio))
    assert info["content_lufs"] == want and abs(info["output_lufs"] - got) <= 1e-9
    if info["max_reduction_db"] == 0:
        assert abs(got - want) <= 0.1
    else:
        assert got <= want                                         # the limiter worked: not above the content's
    assert float(A.true_peak(res.audio)) <= CEIL
    assert res.audio.shape == content.shape and isinstance(res.report, dict)
    fixed = run(solver=None, loudness=-20.0, true_peak_db=-3.0)                        # a LUFS target, the reference's sampler
    assert float(A.true_peak(fixed.audio)) <= 10.0 ** (-3.0 / 20.0)
    if fixed.loudness["max_reduction_db"] == 0:
        assert abs(fixed.loudness["output_lufs"] + 20.0) <= 0.1


def test_report_with_loudness(A, transfer):
    from ldm_amd import metrics
    run, content = transfer
    res = run(solver="dpmpp2m")
    style = dev(R.test_signal(150 * 512, variant=1), content.device)
    plain = metrics.transfer_report(content, res.audio, style)
    rep = metrics.transfer_report(content, res.audio, style, loudness=True)
    assert set(rep) == set(plain) | {"content_lufs", "output_lufs", "style_lufs", "output_true_peak_db"}
    assert all(rep[k] == plain[k] or (np.isnan(rep[k]) and np.isnan(plain[k])) for k in plain)
    assert rep["content_lufs"] == float(A.integrated_loudness(content))
    assert rep["style_lufs"] == float(A.integrated_loudness(style))
    assert abs(rep["output_true_peak_db"] - 20.0 * np.log10(float(A.true_peak(res.audio)))) <= 1e-9
