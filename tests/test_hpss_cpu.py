"""CPU: the harmonic / percussive separation's host side: the yardstick (tests/hpss_ref.py) separates a
sine from clicks, its median is scipy's wherever scipy's reflection is sound, and the argument checks and CLI flags
act before anything touches a device."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hpss_ref as H          # noqa: E402


def test_reference_separates_sine_from_clicks():
    """3 s at 22050 Hz, a 440 Hz sine at 0.5 plus five unit clicks, n_fft 2048, hop 512, window 31, power 2.  The
    restatement gives 0.9931 (harmonic mask at the sine's bin, more than 4 frames from a click) and 0.99999997
    (percussive mask in bins 100..1000 at the click frames)."""
    S, frames = H.sine_clicks_magnitude()
    assert S.shape[0] == 1025 and len(frames) == 5
    mask_h, mask_p = H.hpss_masks(S, 31, 2.0, 1.0)
    h_min, p_min = H.check_sine_clicks_masks(mask_h, mask_p, frames)
    print(f"sine plus clicks (float64 restatement): min mask_h {h_min:.6f}, min mask_p {p_min:.10f}")
    assert h_min >= 0.98
    assert p_min >= 0.99
    assert np.abs(mask_h + mask_p - 1.0).max() <= 1e-12                 # margin 1: the two masks split every bin


@pytest.mark.parametrize("shape,wins", [((2, 7, 5), (1, 3, 31, 63)), ((1, 33, 65), (3, 17, 31)), ((1, 1, 40), (31,)),
                                        ((1, 40, 1), (31,))])
def test_reference_median_is_scipys_where_scipy_reflects_soundly(shape, wins):
    """The yardstick pads the axis itself (numpy "symmetric") and lets scipy filter the padded array.  scipy 1.15's own
    mode="reflect" reads one sample in front of the array when a window reaches 4 axis lengths past the start
    (hpss_ref.scipy_reflect_is_sound); everywhere else the yardstick is the plain scipy call, bit for bit."""
    rng = np.random.default_rng(11)
    for x in (rng.standard_normal(shape).astype(np.float32), np.floor(rng.random(shape) * 4).astype(np.float32)):
        for win in wins:
            for axis in (0, 1):
                got = H.median_filter(x, win, axis)
                assert got.dtype == np.float32 and got.shape == x.shape
                if H.scipy_reflect_is_sound(shape[1 + axis], win):
                    assert np.array_equal(got, H.median_filter_direct(x, win, axis)), (win, axis)
                # the definition itself: the middle of the sorted window of the symmetric continuation
                h = win // 2
                pad = [(0, 0)] * 3
                pad[1 + axis] = (h, h)
                xp = np.moveaxis(np.pad(x, pad, mode="symmetric"), 1 + axis, -1)
                want = np.stack([np.sort(xp[..., i:i + win], axis=-1)[..., h] for i in range(shape[1 + axis])], axis=-1)
                assert np.array_equal(got, np.moveaxis(want, -1, 1 + axis)), (win, axis)


def test_reference_softmask_and_share_conventions():
    X = np.array([0.0, 1.0, 0.0, 2.0, 1e-39], dtype=np.float32)
    Y = np.array([0.0, 0.0, 3.0, 2.0, 0.0], dtype=np.float32)
    for p in (1.0, 1.5, 2.0):
        m = H.softmask(X, Y, p)
        assert m.tolist() == [0.5, 1.0, 0.0, 0.5, 0.5]
    M = np.array([[0.0, 1.0, 2.0, 0.0], [0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
    P = np.array([[1.0], [2.0], [3.0], [4.0]], dtype=np.float32)
    assert H.mel_lohi(M).tolist() == [[1, 3], [0, 0]]
    assert H.mask_mel_share(P, np.ones_like(P), M)[:, 0].tolist() == [1.0, 0.5]
    assert H.mask_mel_share(P, np.zeros_like(P), M)[:, 0].tolist() == [0.0, 0.5]
    half = H.mask_mel_share(P, np.array([[0.0], [1.0], [0.0], [1.0]], dtype=np.float32), M)
    assert abs(half[0, 0] - 2.0 / 8.0) <= 1e-15


def test_cli_flags():
    from models.transfer import parse_args
    base = ["--content", "a.wav", "--style", "b.wav", "--out", "o.wav", "--solver", "dpmpp2m"]
    a = parse_args(base)
    assert a.keep_component is None and a.hpss_kernel == 31 and a.hpss_margin == 1.0
    assert parse_args(base + ["--keep-percussive"]).keep_component == "percussive"
    assert parse_args(base + ["--keep-harmonic"]).keep_component == "harmonic"
    with pytest.raises(SystemExit):
        parse_args(base + ["--keep-percussive", "--keep-harmonic"])         # the two exclude each other
    a = parse_args(base + ["--keep-percussive", "--hpss-kernel", "17", "--hpss-margin", "2"])
    assert a.hpss_kernel == 17 and a.hpss_margin == 2.0
    a = parse_args(base + ["--keep-harmonic", "--hpss-kernel", "31", "9", "--hpss-margin", "1", "3.5"])
    assert a.hpss_kernel == (31, 9) and a.hpss_margin == (1.0, 3.5)
    for bad in (["--hpss-kernel", "30"], ["--hpss-kernel", "65"], ["--hpss-kernel", "3", "5", "7"],
                ["--hpss-margin", "0.5"], ["--hpss-margin", "1", "2", "3"], ["--hpss-margin", "nan"]):
        with pytest.raises(SystemExit):
            parse_args(base + ["--keep-percussive"] + bad)
    with pytest.raises(SystemExit):                                          # needs --solver, like --keep-time
        parse_args(["--content", "a.wav", "--style", "b.wav", "--out", "o.wav", "--keep-percussive"])


def test_bad_arguments_raise_before_any_device_work():
    import models.model as M
    from ldm_amd import audio as A
    from ldm_amd import ops
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval()
    y = torch.zeros(40 * HOP)                                          # CPU tensors: device work would raise RuntimeError
    for comp in ("percussive", "harmonic"):
        with pytest.raises(ValueError, match="keep_component needs a solver"):
            transfer_recording(ldm, y, y, keep_component=comp, solver=None)
    with pytest.raises(ValueError, match="keep_component"):
        transfer_recording(ldm, y, y, keep_component="drums", solver="dpmpp2m")
    with pytest.raises(ValueError, match="win"):
        transfer_recording(ldm, y, y, keep_component="percussive", solver="dpmpp2m", hpss_kernel=30)
    with pytest.raises(ValueError, match="margin"):
        transfer_recording(ldm, y, y, keep_component="percussive", solver="dpmpp2m", hpss_margin=0.5)
    S = torch.zeros(1, 9, 9)
    for win in (0, 30, 65):
        with pytest.raises(ValueError, match="win"):
            ops.median_filter(S, win, 1)
        with pytest.raises(ValueError, match="win"):
            A.hpss_masks(S, kernel_size=win)
    with pytest.raises(ValueError, match="axis"):
        A.median_filter(S, 3, 2)
    for p in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="power"):
            ops.hpss_masks(S, S, p)
    for m in (0.99, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="margin"):
            ops.hpss_masks(S, S, 2.0, m, 1.0)
        with pytest.raises(ValueError, match="margin"):
            A.hpss_masks(S, margin=(1.0, m))
    with pytest.raises(ValueError, match="pair"):
        A.hpss_masks(S, kernel_size=(3, 5, 7))
    with pytest.raises(ValueError, match="component"):
        A.hpss_keep(y, "drums")
    for call in (lambda: ops.median_filter(S, 3, 1), lambda: ops.hpss_masks(S, S),
                 lambda: ops.mask_mel_share(S, S, torch.zeros(2, 9), torch.zeros(2, 2, dtype=torch.int32))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):     # valid arguments on CPU tensors: no fallback
            call()
