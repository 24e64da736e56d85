"""CPU: the host side of the transfer report (ldm_amd/metrics.py): the DCT basis, the chroma
filterbank, the Fréchet distance against scipy.linalg.sqrtm, the yardstick's onset envelope on hand-made numbers, and
the behaviour orderings of tests/test_gpu_metrics.py on the yardstick alone (only orderings it satisfies are asked of
the device)."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_ref as MR      # noqa: E402


@pytest.fixture(scope="module")
def M():
    from ldm_amd import metrics
    return metrics


@pytest.mark.parametrize("n_mfcc,n_mels", [(13, 40), (20, 128), (32, 128), (128, 128)])
def test_dct_basis(M, n_mfcc, n_mels):
    from scipy.fft import dct
    D = M.dct_basis(n_mfcc, n_mels)
    assert D.dtype == np.float64 and D.shape == (n_mfcc, n_mels)
    assert np.abs(D @ D.T - np.eye(n_mfcc)).max() <= 1e-12
    # column m of dct(eye) is the transform of the unit vector e_m: coefficient k is D[k, m]
    assert np.abs(D - dct(np.eye(n_mels), type=2, norm="ortho", axis=0)[:n_mfcc]).max() <= 1e-12
    assert np.abs(D - MR.dct_basis(n_mfcc, n_mels)).max() <= 1e-12
    with pytest.raises(ValueError):
        M.dct_basis(41, 40)


@pytest.mark.parametrize("sr,n_fft", [(22050, 2048), (22050, 512), (16000, 2048)])
def test_chroma_filterbank(M, sr, n_fft):
    cls, wt = M.chroma_filterbank(sr, n_fft)
    rc, rw = MR.chroma_filterbank(sr, n_fft)
    assert cls.dtype == np.int32 and wt.dtype == np.float64 and cls.shape == wt.shape == (n_fft // 2 + 1,)
    assert np.array_equal(cls, rc) and np.abs(wt - rw).max() <= 1e-12
    v = np.arange(n_fft // 2 + 1) * sr / n_fft
    band = (v >= 55.0) & (v <= 5000.0)
    assert band.sum() > 12 and np.array_equal(cls >= 0, band)
    assert np.all(cls[band] < 12) and np.all(cls[~band] == -1) and np.all(wt[~band] == 0)
    lo, hi = wt[band], 1.0 - wt[band]                 # the two weights of an in-band bin
    assert np.all(lo > 0) and np.all(lo <= 1) and np.all(hi >= 0) and np.abs(lo + hi - 1.0).max() <= 1e-15


def test_chroma_filterbank_a440(M):
    """440 Hz lands in class 9 (A) with weight 1: sr and n_fft chosen so that a bin sits exactly on 440 Hz."""
    sr, n_fft = 22000, 2000                             # bin 40 is 440 Hz
    cls, wt = M.chroma_filterbank(sr, n_fft)
    assert cls[40] == 9 and wt[40] == 1.0
    assert cls[80] == 9 and abs(wt[80] - 1.0) <= 1e-12  # the octave above


def spd_pair(seed, n=19):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        A = rng.standard_normal((n, 3 * n))
        out.append((rng.standard_normal(n) * 3.0, A @ A.T / (3 * n) * rng.uniform(0.5, 20.0)))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_frechet_matches_sqrtm(M, seed):
    (m1, C1), (m2, C2) = spd_pair(seed)
    got, want = M.frechet(m1, C1, m2, C2), MR.frechet_sqrtm(m1, C1, m2, C2)
    print(f"frechet {got:.12g} sqrtm {want:.12g} rel {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-9 * want
    assert abs(M.frechet(m2, C2, m1, C1) - got) <= 1e-9 * want     # symmetric


@pytest.mark.parametrize("seed", range(3))
def test_frechet_of_itself(M, seed):
    (m1, C1), _ = spd_pair(seed)
    d = M.frechet(m1, C1, m1, C1)
    assert 0.0 <= d <= 1e-9 * np.trace(C1)
    assert math.isnan(M.frechet(m1, C1, m1, np.full_like(C1, np.nan)))
    # a rank-deficient covariance (fewer frames than coefficients): eigenvalues clamped, still at most 1e-9 tr C
    r = np.random.default_rng(seed).standard_normal((19, 5))
    C = r @ r.T
    assert 0.0 <= M.frechet(m1, C, m1, C) <= 1e-9 * np.trace(C)


def test_reference_onset_by_hand():
    db = np.array([[[0.0, 1.0, -1.0, 3.0],
                    [2.0, 2.0, 5.0, 4.0]]])                                 # [1, 2, 4]
    assert np.array_equal(MR.onset_strength(db, 1), [[0.0, 0.5, 1.5, 2.0]])   # (1+0)/2, (0+3)/2, (4+0)/2
    assert np.array_equal(MR.onset_strength(db, 3), [[0.0, 0.0, 0.0, 2.5]])   # (3+2)/2
    assert np.array_equal(MR.onset_strength(db, 4), np.zeros((1, 4)))


def test_pair_scores_and_moments(M):
    rng = np.random.default_rng(0)
    a, b, w = rng.standard_normal((1, 500)), rng.standard_normal((1, 500)), rng.random((1, 500))
    s = M.PairStats(MR.pair_sums(a, b, w)[0][0])
    mu_a, mu_b = np.average(a[0], weights=w[0]), np.average(b[0], weights=w[0])
    cov = np.average((a[0] - mu_a) * (b[0] - mu_b), weights=w[0])
    want = cov / math.sqrt(np.average((a[0] - mu_a) ** 2, weights=w[0]) * np.average((b[0] - mu_b) ** 2, weights=w[0]))
    assert abs(s.pearson - want) <= 1e-12 and abs(s.pearson - MR.pearson(s.sums)) <= 1e-15
    assert abs(s.cosine - (w * a * b).sum() / math.sqrt((w * a * a).sum() * (w * b * b).sum())) <= 1e-12
    assert abs(s.rms_diff - math.sqrt(np.average((a[0] - b[0]) ** 2, weights=w[0]))) <= 1e-12
    same = M.PairStats(MR.pair_sums(a, a, w)[0][0])
    assert same.pearson == 1.0 and same.cosine == 1.0 and same.rms_diff == 0.0
    for dead in (M.PairStats([0.0] * 7), M.PairStats(MR.pair_sums(np.ones((1, 9)), np.ones((1, 9)))[0][0])):
        assert math.isnan(dead.pearson)                                      # no count / no variance: nan, no exception
    assert math.isnan(M.PairStats([0.0] * 7).cosine) and math.isnan(M.PairStats([0.0] * 7).rms_diff)
    # moments: population mean and covariance of weighted frames; zero count gives nan
    c = rng.standard_normal((5, 300))
    D = np.eye(5)
    sums, _ = MR.mfcc_sums(c[None], D, w[:, :300])
    count, mean, cv = M.moments_from_sums(sums, 5)
    assert abs(count - w[0, :300].sum()) <= 1e-12
    assert np.abs(mean - np.average(c, axis=1, weights=w[0, :300])).max() <= 1e-12
    assert np.abs(cv - np.cov(c, aweights=w[0, :300], bias=True)).max() <= 1e-12
    count, mean, cv = M.moments_from_sums(np.zeros_like(sums), 5)
    assert count == 0 and np.isnan(mean).all() and np.isnan(cv).all()


# ---- the behaviour orderings, on the yardstick alone ------------------------------------------------------------
def test_reference_identity():
    x, s = MR.tone(880.0) + 0.3 * MR.click_train(), MR.noise(2, 0.9)
    keep = np.zeros((MR.N_MELS, 1 + MR.L2S // MR.HOP))
    keep[:40] = 1.0
    rep, (d_c, _, _) = MR.transfer_report(x, x, [s], keep=keep)
    assert abs(rep["onset_corr"] - 1.0) <= 1e-6 and abs(rep["chroma_sim"] - 1.0) <= 1e-6
    assert rep["timbre_out_content"] <= 1e-9 * np.trace(d_c[1])
    assert rep["kept_rms_db"] == 0.0 and rep["changed_rms_db"] == 0.0
    assert abs(rep["timbre_shift"]) <= 1e-9


def test_reference_tone_chroma():
    cls, wt = MR.chroma_filterbank(MR.SR, MR.N_FFT)
    a, b = MR.tone(880.0), MR.tone(880.0 * 2.0 ** 0.5)
    ch = MR.chroma(MR.analyse(a)[0][None], cls, wt)[0]
    assert np.all(ch[:, 2:-2].argmax(axis=0) == 9)
    s = MR.noise(2, 0.9)
    same, moved = MR.transfer_report(a, a, [s])[0], MR.transfer_report(a, b, [s])[0]
    print(f"chroma_sim: tone against itself {same['chroma_sim']:.6f}, against the tritone {moved['chroma_sim']:.6f}")
    assert moved["chroma_sim"] < same["chroma_sim"]


def test_reference_click_onsets():
    c = MR.click_train()
    s = MR.noise(2, 0.9)
    with_tone = MR.transfer_report(c, c + MR.tone(660.0, 0.05), [s])[0]
    shifted = MR.transfer_report(c, MR.click_train(offset=1000 + 5512 // 2), [s])[0]
    print(f"onset_corr: clicks + tone {with_tone['onset_corr']:.4f}, half a period late {shifted['onset_corr']:.4f}")
    assert with_tone["onset_corr"] > shifted["onset_corr"]


def test_reference_timbre_moves_to_the_style():
    rep = MR.transfer_report(MR.noise(1), MR.noise(3, 0.9), [MR.noise(2, 0.9)])[0]
    print("white content, low-passed style, low-passed output of another seed: "
          + ", ".join(f"{k} {rep[k]:.4g}" for k in ("timbre_out_style", "timbre_out_content", "timbre_shift")))
    assert rep["timbre_out_style"] < rep["timbre_out_content"] and rep["timbre_shift"] > 0
