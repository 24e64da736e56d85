"""CPU: the float64 yardstick of the resampler and the silence trim (tests/resample_ref.py) pinned to
scipy.signal.resample_poly, the filter definition's passband and stopband, the trim bounds derived by hand, the host
tap table of ldm_amd.audio, and the fp32-against-float64 margin of the end-to-end test's signal."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as AR   # noqa: E402
import resample_ref as RR   # noqa: E402

RATES = [(44100, 22050), (48000, 22050), (16000, 22050)]


@pytest.mark.parametrize("sr_in,sr_out", RATES)
def test_yardstick_equals_scipy_resample_poly(sr_in, sr_out):
    """resample_poly zero-stuffs by `up`, filters with up * window centred on its middle tap and keeps every
    `down`-th sample: with the up-rate prototype g[m] = h(m / up), |m| <= W up, that is up * the yardstick's sum, so
    the prototype is handed over divided by up."""
    from scipy.signal import resample_poly
    up, down, W, table = RR.taps(sr_in, sr_out)
    fc = min(1.0, up / down) * RR.ROLLOFF
    proto = RR.h(np.arange(-W * up, W * up + 1) / up, fc)
    # the table is the prototype's polyphase split: table[p, j + W] = g[j up - p] (h is even)
    for p in (0, up // 2, up - 1):
        idx = np.arange(-W, W + 1) * up - p
        ok = np.abs(idx) <= W * up
        assert np.abs(table[p][ok] - proto[idx[ok] + W * up]).max() <= 1e-14 and not table[p][~ok].any()
    x = np.random.Generator(np.random.PCG64(11)).standard_normal(2000)
    want = resample_poly(x, up, down, window=proto / up)
    got = RR.resample(x, sr_in, sr_out)
    assert got.shape == want.shape == (RR.n_out(2000, up, down),)
    err = np.abs(got - want).max()
    print(f"{sr_in}->{sr_out}: up {up} down {down} W {W}, max |yardstick - scipy| {err:.3e}")
    assert err <= 1e-10


def test_tap_geometry_and_host_table():
    from ldm_amd import audio
    for (sr_in, sr_out), W in {(44100, 22050): 68, (48000, 22050): 74, (16000, 22050): 34}.items():
        up, down, w, table = audio.resample_taps(sr_in, sr_out)
        assert (up, down, w) == RR.taps(sr_in, sr_out)[:3] and w == W
        assert table.shape == (up, 2 * W + 1) and table.dtype == np.float64 and not table.flags.writeable
        assert np.abs(table - RR.taps(sr_in, sr_out)[3]).max() <= 1e-15
    assert audio.resample_taps(48000, 22050)[0] == 147
    assert audio.resample_taps(48000, 22050) is audio.resample_taps(48000, 22050)   # cached


@pytest.mark.parametrize("sr_in", [44100, 48000])
def test_passband_and_stopband(sr_in):
    """L = sr_in / 4, 600 output samples ignored at each end.  Pass: 100, 1000, 5000 Hz come out as the same sine
    within 1e-7.  Stop: 12, 15, 20 kHz come out below -140 dB (1e-7).  10.4-12 kHz is the transition band."""
    L, sr_out = sr_in // 4, 22050
    up, down = RR.ratio(sr_in, sr_out)
    ns = range(600, RR.n_out(L, up, down) - 600)
    t_out = np.arange(ns.start, ns.stop) / sr_out
    for f in (100.0, 1000.0, 5000.0):
        x = np.sin(2 * np.pi * f * np.arange(L) / sr_in)
        err = np.abs(RR.resample_at(x, sr_in, sr_out, ns) - np.sin(2 * np.pi * f * t_out)).max()
        print(f"{sr_in} pass {f:.0f} Hz: {err:.2e}")
        assert err <= 1e-7
    for f in (12000.0, 15000.0, 20000.0):
        x = np.sin(2 * np.pi * f * np.arange(L) / sr_in)
        peak = np.abs(RR.resample_at(x, sr_in, sr_out, ns)).max()
        print(f"{sr_in} stop {f:.0f} Hz: {20 * np.log10(peak):.1f} dB")
        assert 20 * np.log10(peak) < -140.0


def test_trim_yardstick_on_built_signal():
    y = RR.trim_signal()
    assert len(y) == 16384
    assert RR.trim(y) == RR.TRIM_BOUNDS == (512 * 7, 512 * 26)
    assert RR.trim(np.zeros(5000)) == (0, 0)
    # no frame within 1 dB of the -20 dB threshold: an fp32 evaluation decides every frame the same way
    assert np.abs(RR.trim_db(y) + 20.0).min() > 1.0
    # the same holds for the variant the GPU test clips to a length that is no multiple of 512
    assert RR.trim(y[:13000]) == (3584, 13000)
    assert np.abs(RR.trim_db(y[:13000]) + 20.0).min() > 1.0


def _resample_f32(x, sr_in, sr_out):
    """The yardstick's sum evaluated in float32 (float32 signal, float32 taps, float32 dot)."""
    up, down, W, table = RR.taps(sr_in, sr_out)
    t32 = table.astype(np.float32)
    xp = np.concatenate([np.zeros(W, np.float32), np.asarray(x, np.float32), np.zeros(W + down + 1, np.float32)])
    out = np.empty(RR.n_out(len(x), up, down), np.float32)
    for n in range(len(out)):
        i0, p = divmod(n * down, up)
        out[n] = np.dot(xp[i0:i0 + 2 * W + 1], t32[p])
    return out


def test_dataset_signal_margins():
    """The end-to-end GPU test compares images made from the fp32 resampler's output with images made from the
    yardstick's.  Here: for that test's 44100 Hz recording, no trim frame lies within 1 dB of the threshold (fp32 and
    float64 trim alike), and the float64 log-mel image of the fp32-resampled audio differs from that of the float64-
    resampled audio by at most one grey level on at most 0.1 % of the pixels."""
    stereo, mono = RR.dataset_signals()
    assert np.abs(RR.trim_db(RR.pcm_to_mono(mono)) + 20.0).min() > 1.0
    x = RR.pcm_to_mono(stereo)
    y64 = RR.resample(x, 44100, 22050)
    y32 = _resample_f32(x, 44100, 22050)
    print(f"fp32 against float64 resampling: {np.abs(y32 - y64).max() / np.abs(y64).max():.2e}")
    assert np.abs(RR.trim_db(y64) + 20.0).min() > 1.0
    b64, b32 = RR.trim(y64), RR.trim(y32)
    assert b64 == b32 and b64[1] == len(y64) and 0 < b64[0] < 11008
    n = -(-(b64[1] - b64[0]) // 66150)
    assert n == 3
    img = [AR.quantize(AR.power_to_db(AR.melspectrogram(y[b64[0]:b64[0] + 66150], n_mels=128))) for y in (y64, y32)]
    assert img[0].shape == (128, 130)
    d = np.abs(img[0].astype(np.int32) - img[1].astype(np.int32))
    print(f"pixels that differ: {int((d > 0).sum())} of {d.size}, largest step {int(d.max())}")
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3
