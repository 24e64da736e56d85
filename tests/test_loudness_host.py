"""CPU: the loudness unit's host side: the yardstick itself (tests/loudness_ref.py) against the
standard's table and a full-scale sine, the limiter's bound g <= r, the true-peak envelope of an inter-sample peak, and
the argument checks, which act before anything touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loudness_ref as LR     # noqa: E402


def test_coefficients_match_the_standards_table_at_48k():
    c = LR.coefficients(48000)
    assert np.abs(c[0, :3] - LR.TABLE_48K["shelf_b"]).max() <= 1e-12
    assert np.abs(c[0, 3:] - LR.TABLE_48K["shelf_a"]).max() <= 1e-12
    assert np.array_equal(c[1, :3], [1.0, -2.0, 1.0])
    assert np.abs(c[1, 3:] - LR.TABLE_48K["highpass_a"]).max() <= 1e-12
    from ldm_amd import audio
    for sr in (48000, 22050, 44100):
        k = audio.k_weighting(sr)
        assert k.shape == (2, 5) and k.dtype == np.float64 and np.array_equal(k, LR.coefficients(sr))
    assert audio.loudness_hop(22050) == 2205 == LR.hop_of(22050) and audio.loudness_hop(48000) == 4800
    with pytest.raises(ValueError, match="sample rate"):
        audio.k_weighting(0)


def test_full_scale_997_hz_sine_reads_minus_3_01_lufs():
    """BS.1770's calibration point: a full-scale 997 Hz sine reads -3.01 LUFS (-3.0103 at 48 kHz here; -2.981 at
    22050 Hz, where the bilinear transform puts the shelf's knee a little lower)."""
    l48 = LR.integrated_loudness(LR.sine(997.0, 5.0, 48000), 48000)
    l22 = LR.integrated_loudness(LR.sine(997.0, 5.0, 22050), 22050)
    print(f"997 Hz full scale: {l48:.4f} LUFS at 48 kHz, {l22:.4f} LUFS at 22050 Hz")
    assert abs(l48 + 3.01) <= 0.01
    assert abs(l22 + 2.981) <= 0.01


def test_gates_of_the_reference():
    sr = 22050
    x = LR.gated_signal(sr)
    assert x.size <= 2 * sr
    (integ, n_pass, thr, n_all), l = LR.gate(LR.hop_sums(x, sr), sr)
    assert n_all == x.size // 2205 - 3 and 0 < n_pass < int((l > -70.0).sum()) < n_all
    assert LR.threshold_margin(l, thr) >= 0.1
    assert abs(integ - (-3.0 + 20 * np.log10(0.25))) < 1.0
    short = LR.gate(LR.hop_sums(x[:4 * 2205 - 1], sr), sr)[0]
    assert short[0] == -np.inf and short[1] == 0 and short[3] == 0
    assert LR.gate(LR.hop_sums(np.zeros(sr), sr), sr)[0][:3] == (-np.inf, 0, -np.inf)


@pytest.mark.parametrize("Lh", [0, 7, 110])
def test_gain_never_exceeds_the_per_sample_gain(Lh):
    """g[n] <= r[n]: every m[n + j] in the smoothing sum has r[n] inside its own window, also at both ends (peaks at
    sample 2 and at L - 5), because m lives on the extended range and is not padded with ones itself."""
    sr, L = 22050, 1500
    rng = np.random.default_rng(5)
    x = 0.2 * rng.standard_normal(L)
    x[2], x[L - 5], x[700] = 1.7, -1.4, 2.0
    c = 10.0 ** (-1.0 / 20.0)
    g, r = LR.limiter_gain(x, sr, c, Lh)
    assert r.min() < 0.6 and (g <= r + 1e-14).all() and g.max() <= 1.0 + 1e-14 and g.min() > 0.0
    assert np.abs(g * x).max() <= c * (1 + 1e-12)
    quiet = 0.1 * rng.standard_normal(L)
    gq, rq = LR.limiter_gain(quiet, sr, c, Lh)
    assert (rq == 1.0).all() and (gq == 1.0).all()


def test_envelope_reads_an_inter_sample_peak():
    """A sine at sr / 4 with phase 45 degrees has samples +-A / sqrt(2) only; its true peak is A."""
    sr, A = 22050, 0.8
    x = LR.sine(sr / 4.0, 0.2, sr, amp=A, phase=np.pi / 4.0)
    assert abs(np.abs(x).max() - A / np.sqrt(2.0)) < 1e-9          # sin of arguments up to 7e3: 1e-12 of rounding
    p = LR.envelope(x, sr)[200:-200]
    assert abs(p[1::2].max() - A / np.sqrt(2.0)) < 1e-6            # p[n] covers [n, n + 3/4]: a peak every other sample
    db = 20.0 * np.log10(np.maximum(p[:-1], p[1:]) / A)
    print(f"sr/4 sine: envelope {db.min():.2e} .. {db.max():.2e} dB relative to A")
    assert np.abs(db).max() <= 1e-4
    faded = LR.intersample_sine(sr, A)                               # an abrupt end rings above A; a faded one does not
    assert abs(np.abs(faded).max() - A / np.sqrt(2.0)) < 1e-9
    assert abs(20.0 * np.log10(LR.true_peak(faded, sr) / A)) <= 1e-4


def test_argument_checks_raise_before_any_device_work():
    from ldm_amd import audio
    from data.audio_processor import AudioPreprocessor
    from models.transfer import parse_args, transfer_recording
    y = torch.zeros(4096)
    for kw in ({"target_lufs": float("nan")}, {"target_lufs": float("inf")}, {"target_lufs": -23.0, "ceiling_db": 0.5},
               {"target_lufs": -23.0, "ceiling_db": float("nan")}, {"target_lufs": -23.0, "lookahead_ms": -1.0}):
        with pytest.raises(ValueError, match="target|ceiling|look-ahead"):
            audio.loudness_normalize(y, **kw)
    with pytest.raises(ValueError, match="ceiling"):
        audio.limit(y, ceiling_db=1.0)
    with pytest.raises(ValueError, match="look-ahead"):
        audio.limit(y, lookahead_ms=-0.1)
    with pytest.raises(ValueError, match="fit"):                                   # over the tile's cap
        audio.limit(y, lookahead_ms=1000.0)
    with pytest.raises(ValueError, match="target"):
        AudioPreprocessor().normalize_audio(np.zeros(4096, dtype=np.float32), target_lufs=float("nan"))
    for bad in ("loud", float("nan"), True):
        with pytest.raises(ValueError, match="loudness|target"):
            transfer_recording(None, y, y, loudness=bad)
    with pytest.raises(ValueError, match="ceiling"):
        transfer_recording(None, y, y, loudness="content", true_peak_db=3.0)
    base = ["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"]
    a = parse_args(base)
    assert a.loudness is None and a.true_peak_db == -1.0
    assert parse_args(base + ["--loudness", "content"]).loudness == "content"
    a = parse_args(base + ["--loudness", "-16.5", "--true-peak", "-2"])
    assert a.loudness == -16.5 and a.true_peak_db == -2.0
    for bad in (["--loudness", "quiet"], ["--loudness", "nan"], ["--true-peak", "1"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
    from models import evaluate
    e = ["--content", "a.wav", "--output", "o.wav", "--style", "b.wav"]
    assert evaluate.parse_args(e).loudness is False and evaluate.parse_args(e + ["--loudness"]).loudness is True
