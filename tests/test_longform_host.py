"""CPU: the window plan of ldm_amd.longform against hand-derived cases, the properties of the float64 yardstick
tests/longform_ref.py that the GPU tests lean on, and the command line of models.transfer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import longform_ref as R   # noqa: E402


def plans():
    from ldm_amd import longform
    return (longform.window_plan, R.window_plan)


@pytest.mark.parametrize("which", [0, 1], ids=["package", "yardstick"])
def test_window_plan_hand_cases(which):
    plan = plans()[which]
    # stride 96: windows start at 0, 96, 192 and the third ends at 320 >= 301
    assert plan(301, 128, 32) == (3, 96)
    assert plan(1, 128, 32) == (1, 96)
    assert plan(128, 128, 32) == (1, 96)          # T = frames: one window
    assert plan(129, 128, 32) == (2, 96)          # T = frames + 1: a second window for the last frame
    assert plan(32, 128, 32)[0] == 1              # T <= overlap
    assert plan(128, 128, 0) == (1, 128)
    assert plan(129, 128, 0) == (2, 128)
    assert plan(7752, 512, 64) == (18, 448)       # a 3-minute recording at the defaults
    assert plan(200, 64, 32) == (6, 32)           # overlap = frames / 2 is allowed


@pytest.mark.parametrize("which", [0, 1], ids=["package", "yardstick"])
def test_window_plan_rejects(which):
    plan = plans()[which]
    for bad in ((301, 128, 65), (301, 100, 10), (0, 128, 32), (301, 128, -1), (301, 0, 0)):
        with pytest.raises(ValueError):
            plan(*bad)


def test_every_frame_is_covered_and_by_at_most_two_windows():
    for T, frames, overlap in ((1, 64, 5), (63, 64, 32), (65, 64, 1), (200, 64, 5), (301, 128, 32), (7752, 512, 64)):
        N, stride = R.window_plan(T, frames, overlap)
        cover = np.zeros(T, dtype=int)
        for n in range(N):
            cover[n * stride:n * stride + frames] += 1
        assert cover.min() >= 1 and cover.max() <= 2
        assert ((cover == 2) == R.in_overlap(T, frames, overlap)).all()
        assert N == 1 or (N - 1) * stride < T     # no window lies wholly beyond the recording


@pytest.mark.parametrize("T,frames,overlap", [(200, 64, 5), (200, 64, 32), (65, 64, 1), (301, 128, 32), (63, 64, 32)])
def test_stitch_is_an_exact_partition_of_unity(T, frames, overlap):
    """Windows cut from one dB map that share one ref_db stitch back to that map: the two weights sum to 1."""
    rng = np.random.Generator(np.random.PCG64(11))
    ref = -7.25
    D = ref - 80.0 * rng.random((8, T))
    y = (R.cut(D, frames, overlap, fill=ref) - ref + 80.0) / 80.0
    N = y.shape[0]
    power, db = R.stitch(y[:, None], np.full(N, ref), overlap, T)
    assert np.abs(db - D).max() <= 1e-12
    assert np.abs(power / 10.0 ** (0.1 * D) - 1.0).max() <= 1e-12


def test_overlap_zero_is_concatenation():
    rng = np.random.Generator(np.random.PCG64(12))
    y = rng.random((4, 1, 8, 64)) * 1.4 - 0.2           # some values outside [0, 1]: clamped
    ref = rng.random(4) * 40.0 - 20.0
    _, db = R.stitch(y, ref, 0, 200)
    want = np.concatenate([np.clip(y[n, 0], 0, 1) * 80.0 - 80.0 + ref[n] for n in range(4)], axis=1)[:, :200]
    assert np.array_equal(db, want)


def test_yardstick_windows_refer_to_their_own_maximum():
    P = R.random_power(8, 200, seed=3)
    P[:, 64:128] = 0.0                                  # window 1 of (64, 0) holds no power at all
    x, ref = R.mel_windows(P, 64, 0)
    assert x.shape == (4, 1, 8, 64) and (x[1] == 1.0).all() and abs(ref[1] + 100.0) < 1e-9
    for n in (0, 2, 3):
        assert x[n].max() == 1.0 and x[n].min() == 0.0  # 12 decades: the -80 dB clamp is reached
    assert (x[3, 0, :, 200 - 192:] == 0.0).all()        # the zero padding lies 80 dB under the window's maximum


def test_parse_args():
    from models.transfer import parse_args
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--out", "c.wav"])
    assert (a.content, a.style, a.out, a.checkpoint) == ("a.wav", "b.wav", "c.wav", None)
    assert (a.frames, a.overlap, a.steps, a.eta, a.batch, a.seed) == (512, 64, 100, 0.0, 8, 0)
    a = parse_args(["--content", "a.wav", "--style", "b.wav", "--out", "c.wav", "--checkpoint", "ldm.pth", "--frames",
                    "256", "--overlap", "32", "--steps", "50", "--eta", "0.5", "--batch", "4", "--seed", "9"])
    assert (a.checkpoint, a.frames, a.overlap, a.steps, a.eta, a.batch, a.seed) == ("ldm.pth", 256, 32, 50, 0.5, 4, 9)
    for missing in ("--content", "--style", "--out"):
        argv = [v for k in ("--content", "--style", "--out") if k != missing for v in (k, "x.wav")]
        with pytest.raises(SystemExit):
            parse_args(argv)
