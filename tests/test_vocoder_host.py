"""CPU: the content-anchored vocoder's host side: the float64 yardstick's own identities
(tests/vocoder_ref.py), the properties of the seeds the GPU tests rely on, the per-bin filter table, the argument
checks (raised before anything touches a device) and the CLI flags."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R          # noqa: E402
import vocoder_ref as V        # noqa: E402


@pytest.fixture(scope="module")
def cases():
    return {name: V.gain_case(name) for name in V.CASES}


@pytest.mark.parametrize("case", list(V.CASES))
def test_unchanged_mel_is_the_identity(cases, case):
    c = cases[case]
    A, P0, a, _ = V.mel_gain_target(c["C"], c["Mc"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB, 6.0)
    assert np.abs(V.bin_gain(c["Mc"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB) - 1.0).max() <= 1e-12
    assert np.abs(A - np.abs(c["C"])).max() <= 1e-12 * np.abs(c["C"]).max()
    assert a.min() >= 1.0 - 1e-12
    assert (P0[c["zero"]] == 1.0).all() and np.abs(np.abs(P0) - 1.0).max() <= 1e-12
    want = R.istft(c["C"], n_fft=c["n_fft"])
    for k in (0, 1, 3):
        y = V.griffinlim_anchored(A, P0, a, k, n_fft=c["n_fft"])
        assert np.abs(y - want).max() <= 1e-10 * np.abs(want).max()
    y1 = V.griffinlim_anchored(A, P0, np.ones_like(a), 3, n_fft=c["n_fft"])     # a == 1: P0 itself, any n_iter
    assert np.array_equal(y1, V.griffinlim_anchored(A, P0, np.ones_like(a), 0, n_fft=c["n_fft"]))


@pytest.mark.parametrize("case", list(V.CASES))
def test_no_anchor_is_plain_griffinlim_from_the_content_phase(cases, case):
    c = cases[case]
    A, P0, a, _ = V.mel_gain_target(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB, 0.0)
    assert (a == 0).all()
    for k in (1, 3):
        assert np.array_equal(V.griffinlim_anchored(A, P0, a, k, n_fft=c["n_fft"]),
                              R.griffinlim(A, P0, k, n_fft=c["n_fft"]))


@pytest.mark.parametrize("case", list(V.CASES))
def test_seed_properties_the_gpu_tests_rely_on(cases, case):
    c = cases[case]
    g = V.bin_gain(c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB)
    assert (g == 10.0 ** (V.MAX_GAIN_DB / 10.0)).any() and c["zero"].any()          # the clamp and the (1, 0) phase are met
    for res in (None, c["R"]):
        A, P0, a, pre = V.mel_gain_target(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB, 6.0, res)
        near = (np.abs(pre) < 1e-3) | (np.abs(pre - 1.0) < 1e-3)
        assert near.mean() <= 0.02
        assert ((a > 0) & (a < 1)).mean() > 0.1 and (a == 0).any()
    A, P0, a, _ = V.mel_gain_target(c["C"], c["Mo"], c["Mc"], c["M"], c["eps"], V.MAX_GAIN_DB, 6.0)
    assert V.griffinlim_anchored(A, P0, a, 4, n_fft=c["n_fft"], return_min_blend=True)[1] >= 1e-3


@pytest.mark.parametrize("n_fft", [512, 2048])
def test_per_bin_filter_table(n_fft):
    from ldm_amd import audio as A
    Wn, mlohi = A._gain_host(22050, n_fft, 128)
    M = R.mel_filterbank(22050, n_fft, 128)
    F = n_fft // 2 + 1
    assert Wn.shape == (128, F) and Wn.dtype == np.float32 and mlohi.shape == (F, 2) and mlohi.dtype == np.int32
    col = M.sum(axis=0)
    assert (mlohi[0] == 0).all() and col[0] == 0                       # DC: no filter, gain 1
    for f in range(F):
        lo, hi = mlohi[f]
        assert 0 <= lo <= hi <= 128 and hi - lo <= 3
        assert not Wn[:lo, f].any() and not Wn[hi:, f].any()
        if col[f] > 0:
            assert np.abs(Wn[:, f] - M[:, f] / col[f]).max() <= 1e-7 and abs(Wn[lo:hi, f].sum(dtype=np.float64) - 1) <= 1e-6
        else:
            assert lo == hi


def test_bad_arguments_raise_before_any_device_work():
    import models.model as M
    from ldm_amd import audio as A
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval()
    y = torch.zeros(40 * HOP)                                          # CPU tensors: device work would raise RuntimeError
    with pytest.raises(ValueError, match="vocoder"):
        transfer_recording(ldm, y, y, vocoder="wavenet")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="max_gain_db"):
            transfer_recording(ldm, y, y, vocoder="content", max_gain_db=bad)
    for bad in (float("nan"), float("-inf")):
        with pytest.raises(ValueError, match="anchor_db"):
            transfer_recording(ldm, y, y, vocoder="content", anchor_db=bad)
    with pytest.raises(ValueError, match="max_gain_db"):
        transfer_recording(ldm, y, y, max_gain_db=-3.0)               # checked whatever the vocoder
    C = torch.zeros(1, 257, 5, dtype=torch.complex64)
    mel = torch.ones(1, 128, 5)
    with pytest.raises(ValueError, match="max_gain_db"):
        A.mel_gain_target(C, mel, mel, 1e-3, max_gain_db=-1.0)
    with pytest.raises(ValueError, match="anchor_db"):
        A.mel_gain_target(C, mel, mel, 1e-3, anchor_db=float("nan"))
    with pytest.raises(ValueError, match="anchor_db"):
        A.mel_to_audio_content(mel, torch.zeros(1, 4 * 128), anchor_db=float("inf"))
    with pytest.raises(ValueError, match="both or neither"):
        A.griffinlim(torch.ones(1, 257, 5), anchor=torch.ones(1, 257, 5))
    with pytest.raises(ValueError, match="both or neither"):
        A.griffinlim(torch.ones(1, 257, 5), anchor_phase=C)


def test_cli_flags():
    from models.transfer import parse_args
    base = ["--content", "a.wav", "--style", "b.wav", "--out", "o.wav"]
    a = parse_args(base)
    assert a.vocoder == "griffinlim" and a.max_gain_db == 40.0 and a.anchor_db == 6.0 and a.residual is True
    a = parse_args(base + ["--vocoder", "content", "--max-gain-db", "20", "--anchor-db", "0", "--no-residual"])
    assert a.vocoder == "content" and a.max_gain_db == 20.0 and a.anchor_db == 0.0 and a.residual is False
    for bad in (["--vocoder", "wavenet"], ["--max-gain-db", "-1"], ["--max-gain-db", "nan"], ["--anchor-db", "inf"]):
        with pytest.raises(SystemExit):
            parse_args(base + bad)
