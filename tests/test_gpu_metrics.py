"""GPU: the transfer report (csrc/metrics.hip, ldm_amd/metrics.py) against tests/metrics_ref.py: the
four feature kernels against float64 with derived bounds, their bitwise repeatability and batch independence, the
report's behaviour through orderings and identities that the yardstick itself satisfies (tests/test_metrics_cpu.py),
and transfer_recording(report=True), --report and python -m models.evaluate."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R         # noqa: E402
import metrics_ref as MR      # noqa: E402

pytestmark = pytest.mark.gpu

U32, U64 = 2.0 ** -24, 2.0 ** -52
DENORMAL = float(np.finfo(np.float32).smallest_subnormal)
TS, BS = (1, 63, 257, 300), (1, 3)
KEYS = ("onset_corr", "chroma_sim", "timbre_out_style", "timbre_out_content", "timbre_content_style", "timbre_shift")
KEEP_KEYS = ("kept_rms_db", "changed_rms_db")


@pytest.fixture(scope="module")
def ops():
    from ldm_amd import ops
    return ops


@pytest.fixture(scope="module")
def M():
    from ldm_amd import metrics
    return metrics


def dev(a, cuda, dtype=torch.float32):
    return torch.from_numpy(np.array(a)).to(dtype).to(cuda)       # a copy: the cached tables are read-only


def weights(kind, shape, rng):
    """None, random in [0, 1], or random with runs of zeros."""
    if kind == "none":
        return None
    w = rng.random(shape).astype(np.float32)
    if kind == "runs":
        flat = w.reshape(shape[0], -1)
        n = flat.shape[1]
        flat[:, : n // 3] = 0.0
        flat[:, n // 2: n // 2 + max(1, n // 5)] = 0.0
    return w


def log_mel(rng, B, n_mels, T):
    return (rng.random((B, n_mels, T)) * 80.0 - 80.0).astype(np.float32)


# ---- 1. onset strength -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
def test_onset_strength(ops, cuda, T, B):
    """Every term max(0, a - b) is one rounding, the n_mels non-negative terms add in n_mels - 1 roundings and the mean
    is one division: at most (n_mels + 2) 2^-24 relative, nothing cancels."""
    rng = np.random.default_rng(100 * T + B)
    for n_mels in (128, 40):
        db = log_mel(rng, B, n_mels, T)
        d = dev(db, cuda)
        for lag in (1, 3):
            got = ops.onset_strength(d, lag)
            want = MR.onset_strength(db, lag)
            assert got.shape == (B, T) and got.dtype == torch.float32
            err = np.abs(got.cpu().numpy().astype(np.float64) - want)
            assert np.all(err <= (n_mels + 2) * U32 * want + DENORMAL), (n_mels, lag, float(err.max()))
            assert bool((got[:, :lag] == 0).all())                      # T <= lag: all zeros
            assert torch.equal(got, ops.onset_strength(d, lag))         # repeatable
            if B > 1:
                for b in range(B):
                    assert torch.equal(got[b:b + 1], ops.onset_strength(d[b:b + 1].contiguous(), lag))


def test_onset_strength_arguments(ops, M, cuda):
    d = dev(log_mel(np.random.default_rng(0), 1, 8, 9), cuda)
    assert torch.equal(M.onset_strength(d[0]), ops.onset_strength(d, 1)[0])
    for lag in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="lag"):
            ops.onset_strength(d, lag)
    with pytest.raises(ValueError, match="db"):
        ops.onset_strength(d[0], 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.onset_strength(d.cpu(), 1)


# ---- 2. chroma -------------------------------------------------------------------------------------------------
def chroma_bound(cls):
    """With K in-band bins: a term w P is one rounding and (1 - w) P two, a class adds at most K non-negative terms, so
    a class sum is within (K + 1) u of its value (u = 2^-24).  The norm: twelve squares (2 (K + 1) u + u each), eleven
    additions of non-negative numbers (11 u), a square root (halves the relative error, one rounding), together within
    (K + 1) u + 7 u; the division adds u.  The quotient, at most 1, is therefore within (2 K + 11) u to first order;
    (2 K + 16) u leaves room for the second-order terms."""
    return (2 * int((cls >= 0).sum()) + 16) * U32


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
def test_chroma(ops, M, cuda, T, B):
    rng = np.random.default_rng(200 * T + B)
    for n_fft in (512, 2048):
        F = n_fft // 2 + 1
        cls, wt = M.chroma_filterbank(22050, n_fft)
        wt32 = wt.astype(np.float32)                                     # the table the device holds
        P = (rng.random((B, F, T)) ** 3 * 50.0).astype(np.float32)
        zero = np.arange(T) % 5 == 0                                     # all-zero frames
        outside = np.arange(T) % 7 == 3                                  # frames with power outside the band only
        P[:, :, zero] = 0.0
        P[:, :, outside] *= (cls < 0)[None, :, None]
        d = dev(P, cuda)
        got = ops.chroma(d, dev(cls, cuda, torch.int32), dev(wt32, cuda))
        want = MR.chroma(P, cls, wt32.astype(np.float64))
        assert got.shape == (B, 12, T) and got.dtype == torch.float32
        g = got.cpu().numpy()
        err = float(np.abs(g - want).max())
        assert err <= chroma_bound(cls), (n_fft, err, chroma_bound(cls))
        assert np.all(g[:, :, zero | outside] == 0.0)                    # exact zeros
        live = ~(zero | outside)
        if live.any():
            assert np.abs(np.sqrt((g[:, :, live].astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 16 * U32
        assert torch.equal(got, M.chroma(d, 22050, n_fft))               # the cached tables are these tables
        assert torch.equal(got, M.chroma(d, 22050, n_fft))               # repeatable
        if B > 1:
            for b in range(B):
                assert torch.equal(got[b:b + 1], M.chroma(d[b:b + 1].contiguous(), 22050, n_fft))


def test_chroma_arguments(ops, M, cuda):
    cls, wt = M.chroma_filterbank(22050, 512)
    c, w = dev(cls, cuda, torch.int32), dev(wt, cuda)
    P = dev(np.ones((1, 257, 4), dtype=np.float32), cuda)
    with pytest.raises(ValueError, match="cls and wt"):
        ops.chroma(P, c[:100], w)
    with pytest.raises(RuntimeError, match="int32"):
        ops.chroma(P, c.long(), w)
    with pytest.raises(ValueError, match="P"):
        ops.chroma(P[0], c, w)
    tiny = ops.chroma(P * 1e-30, c, w)                                   # a norm below the smallest normal fp32
    assert bool((tiny == 0).all())


# ---- 3. MFCC moments and pair sums -----------------------------------------------------------------------------
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
def test_mfcc_moments(ops, M, cuda, T, B):
    """Each entry within (T + n_mels + 8) 2^-52 S_abs of float64, S_abs the sum of the absolute terms the yardstick
    adds for that entry, the terms |D[k, m] db[m, t]| of the coefficients inside it included: a coefficient is a sum of
    n_mels products (n_mels 2^-53 of their absolute sum), a product of two coefficients twice that, and the frames add
    T more roundings: (2 n_mels + T + 3) 2^-53 of S_abs in all."""
    rng = np.random.default_rng(300 * T + B)
    for n_mels, n_mfccs in ((128, (13, 20, 32)), (40, (13,))):
        db = log_mel(rng, B, n_mels, T)
        d = dev(db, cuda)
        for n in n_mfccs:
            D = MR.dct_basis(n, n_mels)
            Dd = dev(D, cuda, torch.float64)
            for kind in ("none", "random", "runs"):
                w = weights(kind, (B, T), rng)
                wd = None if w is None else dev(w, cuda)
                got = ops.mfcc_moments(d, Dd, wd)
                want, mags = MR.mfcc_sums(db, D, w)
                assert got.shape == want.shape and got.dtype == torch.float64
                err = np.abs(got.cpu().numpy() - want)
                bound = (T + n_mels + 8) * U64 * mags
                assert np.all(err <= bound), (n_mels, n, kind, float((err / np.maximum(bound, 1e-300)).max()))
                assert torch.equal(got, ops.mfcc_moments(d, Dd, wd))
                if B > 1:
                    for b in range(B):
                        one = ops.mfcc_moments(d[b:b + 1].contiguous(), Dd, None if wd is None else wd[b:b + 1].contiguous())
                        assert torch.equal(got[b:b + 1], one)


def test_mfcc_moments_wrapper(ops, M, cuda):
    rng = np.random.default_rng(7)
    db, w = log_mel(rng, 2, 128, 150), weights("runs", (2, 150), rng)
    count, mean, cov = M.mfcc_moments(dev(db, cuda), 20, dev(w, cuda))
    rc, rm, rv = MR.moments_from_sums(MR.mfcc_sums(db, MR.dct_basis(20, 128), w)[0], 20)
    assert mean.dtype == np.float64 and cov.shape == (20, 20)
    assert abs(count - rc) <= 1e-12 * rc and np.abs(mean - rm).max() <= 1e-9 and np.abs(cov - rv).max() <= 1e-9 * np.trace(rv)
    count, mean, cov = M.mfcc_moments(dev(db[0], cuda), 13, dev(np.zeros(150, dtype=np.float32), cuda))
    assert count == 0 and np.isnan(mean).all() and np.isnan(cov).all()    # no frame: nan, no exception
    d = dev(db, cuda)
    with pytest.raises(ValueError, match="n_mfcc"):
        ops.mfcc_moments(d, dev(np.zeros((33, 128)), cuda, torch.float64))
    with pytest.raises(ValueError, match="weight"):
        ops.mfcc_moments(d, dev(MR.dct_basis(13, 128), cuda, torch.float64), dev(w[:, :9], cuda))
    with pytest.raises(RuntimeError, match="float64"):
        ops.mfcc_moments(d, dev(MR.dct_basis(13, 128), cuda))


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("n", (1, 255, 4097))
def test_pair_stats(ops, cuda, n, B):
    """Each sum within (n + 8) 2^-52 of the sum of its absolute terms: a term is at most three roundings (the product
    of two fp32 values is exact in float64), the slice partials and their combination add fewer than n."""
    rng = np.random.default_rng(400 * n + B)
    a = (rng.standard_normal((B, n)) * 30.0).astype(np.float32)
    b = (a + rng.standard_normal((B, n)).astype(np.float32) * (rng.random((B, n)) < 0.7)).astype(np.float32)
    ad, bd = dev(a, cuda), dev(b, cuda)
    for kind in ("none", "random", "runs"):
        w = weights(kind, (B, n), rng)
        wd = None if w is None else dev(w, cuda)
        got = ops.pair_stats(ad, bd, wd)
        want, mags = MR.pair_sums(a, b, w)
        assert got.shape == (B, 7) and got.dtype == torch.float64
        err = np.abs(got.cpu().numpy() - want)
        assert np.all(err <= (n + 8) * U64 * mags), (kind, err, mags)
        assert torch.equal(got, ops.pair_stats(ad, bd, wd))
        same = ops.pair_stats(ad, ad, wd)
        assert torch.equal(same[:, 3], same[:, 4]) and torch.equal(same[:, 3], same[:, 5]) and bool((same[:, 6] == 0).all())
        if B > 1:
            for i in range(B):
                one = ops.pair_stats(ad[i:i + 1].contiguous(), bd[i:i + 1].contiguous(),
                                     None if wd is None else wd[i:i + 1].contiguous())
                assert torch.equal(got[i:i + 1], one)


def test_pair_stats_wrapper(ops, M, cuda):
    rng = np.random.default_rng(9)
    a, b = rng.standard_normal((12, 50)).astype(np.float32), rng.standard_normal((12, 50)).astype(np.float32)
    s = M.pair_stats(dev(a, cuda), dev(b, cuda))
    want = MR.pair_sums(a.reshape(1, -1), b.reshape(1, -1))[0][0]
    assert abs(s.pearson - MR.pearson(want)) <= 1e-12 and abs(s.pearson - np.corrcoef(a.ravel(), b.ravel())[0, 1]) <= 1e-6
    z = M.pair_stats(dev(a, cuda), dev(b, cuda), torch.zeros(12, 50, device=cuda))
    assert math.isnan(z.pearson) and math.isnan(z.cosine) and math.isnan(z.rms_diff)
    assert math.isnan(M.pair_stats(torch.ones(9, device=cuda), torch.ones(9, device=cuda)).pearson)
    with pytest.raises(ValueError, match="one shape"):
        M.pair_stats(dev(a, cuda), dev(b[:, :9], cuda))
    with pytest.raises(ValueError, match="non-empty"):
        ops.pair_stats(dev(a[0], cuda), dev(b[0], cuda))


# ---- 4. behaviour: orderings and identities the yardstick satisfies ----------------------------------------------
@pytest.fixture(scope="module")
def style_wave(cuda):
    return dev(MR.noise(2, 0.9), cuda)


def show(name, rep):
    print(name + ": " + ", ".join(f"{k} {v:.6g}" for k, v in rep.items()))


def test_report_of_a_signal_with_itself(M, cuda, style_wave):
    xn = MR.tone(880.0) + 0.3 * MR.click_train()
    x = dev(xn, cuda)
    T = 1 + MR.L2S // MR.HOP
    keep = np.zeros((MR.N_MELS, T), dtype=np.float32)
    keep[:40] = 1.0
    rep = M.transfer_report(x, x, style_wave, keep=torch.from_numpy(keep))
    ref, (d_c, _, _) = MR.transfer_report(xn, xn, [MR.noise(2, 0.9)], keep=keep)
    show("x against x (device)", rep)
    show("x against x (float64)", ref)
    assert tuple(rep) == KEYS + KEEP_KEYS and all(type(v) is float for v in rep.values())
    assert abs(rep["onset_corr"] - 1.0) <= 1e-6 and abs(rep["chroma_sim"] - 1.0) <= 1e-6
    assert rep["timbre_out_content"] <= 1e-9 * np.trace(d_c[1])
    assert rep["kept_rms_db"] == 0.0
    assert tuple(M.transfer_report(x, x, [style_wave, style_wave])) == KEYS      # no keep: no keep keys; a list of styles


def test_report_tone_chroma(M, cuda, style_wave):
    a, b = dev(MR.tone(880.0), cuda), dev(MR.tone(880.0 * 2.0 ** 0.5), cuda)
    from ldm_amd import ops
    ch = M.chroma(ops.stft(a.unsqueeze(0), 2048, None, "power"))[0]
    assert bool((ch[:, 2:-2].argmax(dim=0) == 9).all())                  # 880 Hz is an A
    same, moved = M.transfer_report(a, a, style_wave), M.transfer_report(a, b, style_wave)
    print(f"chroma_sim: tone against itself {same['chroma_sim']:.6f}, against the tritone {moved['chroma_sim']:.6f}")
    assert moved["chroma_sim"] < same["chroma_sim"]


def test_report_click_onsets(M, cuda, style_wave):
    c = MR.click_train()
    with_tone = M.transfer_report(dev(c, cuda), dev(c + MR.tone(660.0, 0.05), cuda), style_wave)
    shifted = M.transfer_report(dev(c, cuda), dev(MR.click_train(offset=1000 + 5512 // 2), cuda), style_wave)
    print(f"onset_corr: clicks + tone {with_tone['onset_corr']:.4f}, half a period late {shifted['onset_corr']:.4f}")
    assert with_tone["onset_corr"] > shifted["onset_corr"]


def test_report_timbre_moves_to_the_style(M, cuda, style_wave):
    rep = M.transfer_report(dev(MR.noise(1), cuda), dev(MR.noise(3, 0.9), cuda), style_wave)
    show("white content, low-passed output", rep)
    assert rep["timbre_out_style"] < rep["timbre_out_content"] and rep["timbre_shift"] > 0


def test_report_arguments(M, cuda, style_wave):
    x = dev(MR.tone(880.0), cuda)
    with pytest.raises(ValueError, match="one length"):
        M.transfer_report(x, x[:-5], style_wave)
    with pytest.raises(ValueError, match="keep"):
        M.transfer_report(x, x, style_wave, keep=torch.zeros(128, 3))
    with pytest.raises(ValueError, match="n_mfcc"):
        M.transfer_report(x, x, style_wave, n_mfcc=40)
    with pytest.raises(ValueError, match="no style"):
        M.transfer_report(x, x, [])
    silent = M.transfer_report(torch.zeros_like(x), torch.zeros_like(x), style_wave)   # nan, never an exception
    assert math.isnan(silent["onset_corr"]) and tuple(silent) == KEYS


# ---- 5. transfer_recording, the command lines --------------------------------------------------------------------
@pytest.fixture(scope="module")
def transfer(cuda):
    import models.model as Mod
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    model = Mod.LDM(32, pretrained_path="").eval().to(cuda)
    frames, overlap, T_total = 128, 32, 224                                 # two windows: [0, 128) and [96, 224)
    L = (T_total - 1) * HOP
    y = R.test_signal(L).astype(np.float32)
    y[np.arange(20, T_total - 1, 37) * HOP] += 1.0                         # a few drum hits
    content = dev(y, cuda)
    style = dev(R.test_signal(150 * HOP, variant=1), cuda)
    kw = dict(frames=frames, overlap=overlap, num_timesteps=2, n_iter=2, nnls_iters=2, seed=4, solver="dpmpp2m")

    def run(**extra):
        return transfer_recording(model, content, style, **dict(kw, **extra))
    return run, content, style


def finite_floats(rep, keys):
    return tuple(rep) == keys and all(type(v) is float and math.isfinite(v) for v in rep.values())


def test_transfer_recording_report(M, transfer):
    run, content, style = transfer
    plain, scored = run(), run(report=True)
    assert not hasattr(plain, "report")
    show("transfer (untrained weights)", scored.report)
    assert finite_floats(scored.report, KEYS)
    assert torch.equal(plain.audio, scored.audio) and torch.equal(plain.mel_power, scored.mel_power)
    assert scored.report == M.transfer_report(content, scored.audio, style)
    kept, kept_plain = run(report=True, keep_component="percussive"), run(keep_component="percussive")
    show("transfer keeping the percussive part", kept.report)
    assert finite_floats(kept.report, KEYS + KEEP_KEYS)
    assert torch.equal(kept.audio, kept_plain.audio)
    from ldm_amd import audio
    mask = audio.hpss_keep(content, "percussive")                          # the mask the transfer used
    assert kept.report == M.transfer_report(content, kept.audio, style, keep=mask)


def write_wavs(tmp_path, cuda):
    from data.audio_processor import save_wav
    from models.transfer import HOP
    L = 150 * HOP
    paths = {}
    for name, sig in (("content", R.test_signal(L)), ("output", R.test_signal(L, variant=2)),
                      ("style", R.test_signal(L + 777, variant=1))):
        paths[name] = str(tmp_path / f"{name}.wav")
        save_wav(paths[name], 0.5 * sig, 22050)
    return paths


def same_reports(a, b):
    return tuple(a) == tuple(b) and all(x == y or (math.isnan(x) and math.isnan(y)) for x, y in zip(a.values(), b.values()))


def test_evaluate_files(M, cuda, tmp_path, capsys):
    from data.audio_processor import AudioPreprocessor
    from ldm_amd import longform
    from models import evaluate
    from models.transfer import HOP
    p = write_wavs(tmp_path, cuda)
    ap = AudioPreprocessor()
    c, o, s = (ap.load_audio_native(p[k])[0] for k in ("content", "output", "style"))
    out = str(tmp_path / "scores.json")
    assert evaluate.main(["--content", p["content"], "--output", p["output"], "--style", p["style"], "--report", out]) == 0
    rep = json.loads(open(out).read())
    assert same_reports(rep, M.transfer_report(c, o, s)) and finite_floats(rep, KEYS)
    capsys.readouterr()
    assert evaluate.main(["--content", p["content"], "--output", p["output"], "--style", p["style"], p["style"],
                          "--keep-time", "0:1.5", "--keep-band", "0:300"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    keep = longform.keep_mask(1 + c.numel() // HOP, 128, 22050, times=[(0.0, 1.5)], bands=[(0.0, 300.0)])
    assert same_reports(rep, M.transfer_report(c, o, [s, s], keep=keep)) and tuple(rep) == KEYS + KEEP_KEYS
    with pytest.raises(SystemExit, match="one length"):
        evaluate.main(["--content", p["content"], "--output", p["style"], "--style", p["style"]])


def test_transfer_cli_report(cuda, tmp_path, capsys):
    from models import transfer as Tr
    p = write_wavs(tmp_path, cuda)
    common = ["--content", p["content"], "--style", p["style"], "--out", str(tmp_path / "o.wav"), "--frames", "128",
              "--overlap", "32", "--steps", "2", "--solver", "dpmpp2m", "--keep-time", "0:1"]
    assert Tr.parse_args(common).report is None
    assert Tr.main(common + ["--report"]) == 0
    rep = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert tuple(rep) == KEYS + KEEP_KEYS and all(type(v) is float for v in rep.values())
    Tr.write_report(rep, str(tmp_path / "r.json"))
    assert same_reports(json.loads(open(tmp_path / "r.json").read()), rep)
    assert Tr.parse_args(common + ["--report", "x.json"]).report == "x.json"
