"""GPU: harmonic / percussive separation (csrc/hpss.hip) against tests/hpss_ref.py: the running median
bit for bit against scipy on both axes, the soft masks and the mel energy share against float64, the separation of a
sine from clicks, and transfer_recording's keep_component against the same call with the mask passed as keep=."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import audio_ref as R         # noqa: E402
import hpss_ref as H          # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24                # one fp32 rounding of a value in [0, 1]
# The largest |device - float64| of the masks at power 1.5 over MASK_SHAPES and both margin sets, measured on an MI355X
# (powf's accuracy is not derivable here); the test allows 4 times it for other inputs.
POWF_MEASURED = 9.11e-8


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


def data_kinds(shape, seed):
    """random, 4-level (every window holds ties), all zeros, and signed zeros with denormals among small values."""
    rng = np.random.default_rng(seed)
    special = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 3e-39, 1.0, -1.0], dtype=np.float32), size=shape)
    return {"random": rng.standard_normal(shape).astype(np.float32),
            "levels": np.floor(rng.random(shape) * 4).astype(np.float32),
            "zeros": np.zeros(shape, dtype=np.float32),
            "special": special.astype(np.float32)}


def median_cases(ops):
    tile_t, tile_f = ops.median_tile(1), ops.median_tile(0)
    assert tile_t >= 64 and tile_f >= 4
    cases = [((1, 1025, 1), (31,)), ((1, 1, 40), (31,)), ((2, 7, 5), (31, 63)), ((1, 1025, 70), (3, 17, 31))]
    cases += [((1, 33, T), (31,)) for T in sorted({63, 64, 65, 257, tile_t - 1, tile_t + 1})]
    cases += [((1, F, 33), (31,)) for F in sorted({tile_f - 1, tile_f + 1})]       # the frequency pass's tile edge
    return cases


# ---- 1. the median --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "levels", "zeros", "special"])
def test_median_is_scipys_bitwise(ops, cuda, kind):
    for n, (shape, wins) in enumerate(median_cases(ops)):
        x = data_kinds(shape, 100 + n)[kind]
        xd = dev(x, cuda)
        for win in wins + (1,):
            for axis in (0, 1):
                got = ops.median_filter(xd, win, axis)
                want = torch.from_numpy(H.median_filter(x, win, axis))
                assert torch.equal(got.cpu(), want), (kind, shape, win, axis)
                if win == 1:
                    assert torch.equal(got, xd)
        assert torch.equal(xd.cpu(), torch.from_numpy(x))                         # the input is left alone


def test_median_wrapper_and_out(A, ops, cuda):
    x = data_kinds((3, 40, 70), 7)["levels"]
    xd = dev(x, cuda)
    out = torch.full_like(xd, -7.0)
    assert ops.median_filter(xd, 17, 1, out=out) is out
    assert torch.equal(out.cpu(), torch.from_numpy(H.median_filter(x, 17, 1)))
    assert torch.equal(A.median_filter(xd[1], 9, 0).cpu(), torch.from_numpy(H.median_filter(x[1], 9, 0)))
    nc = xd.transpose(1, 2)                                                        # a non-contiguous view is copied
    assert torch.equal(ops.median_filter(nc, 5, 1).cpu(),
                       torch.from_numpy(H.median_filter(np.ascontiguousarray(x.transpose(0, 2, 1)), 5, 1)))


def test_median_bad_arguments(ops, cuda):
    x = torch.zeros((1, 9, 9), device=cuda)
    for win in (0, 30, 65):
        with pytest.raises(ValueError, match="win"):
            ops.median_filter(x, win, 1)
    with pytest.raises(ValueError, match="axis"):
        ops.median_filter(x, 3, 2)
    with pytest.raises(ValueError, match="alias"):
        ops.median_filter(x, 3, 1, out=x)
    buf = torch.zeros(2 * 81 - 9, device=cuda)
    with pytest.raises(ValueError, match="alias"):                                 # a partial overlap is an alias too
        ops.median_filter(buf[:81].view(1, 9, 9), 3, 0, out=buf[72:153].view(1, 9, 9))
    with pytest.raises(ValueError, match="out"):
        ops.median_filter(x, 3, 1, out=torch.zeros((1, 9, 8), device=cuda))
    with pytest.raises(ValueError, match=r"\[B, F, T\]"):
        ops.median_filter(x[0], 3, 1)
    with pytest.raises(RuntimeError, match="expected"):
        ops.median_filter(x.double(), 3, 1)
    # the C entry reports the same errors through its error state
    from ldm_amd import _lib as L
    s = ops.stream_handle()
    y = torch.empty_like(x)
    for args, what in (((x.data_ptr(), 1, 9, 9, 1, 30, y.data_ptr(), s), "win"),
                       ((x.data_ptr(), 1, 9, 9, 1, 65, y.data_ptr(), s), "win"),
                       ((x.data_ptr(), 1, 9, 9, 2, 3, y.data_ptr(), s), "axis"),
                       ((x.data_ptr(), 0, 9, 9, 1, 3, y.data_ptr(), s), "shape"),
                       ((x.data_ptr(), 1, 9, 9, 1, 3, None, s), "null"),
                       ((x.data_ptr(), 1, 9, 9, 1, 3, x.data_ptr(), s), "alias")):
        with pytest.raises(L.LDMError, match=what):
            L.call("ldm_median_filter", *args)


# ---- 2. the soft masks ----------------------------------------------------------------------------------------
MASK_SHAPES = ((1, 1025, 70), (2, 7, 5))


def mask_inputs(shape, seed):
    """Two non-negative "medians" with a spread of ratios, exact zeros in one, the other and both, and denormals."""
    rng = np.random.default_rng(seed)
    h = (rng.random(shape) ** 3 * 10.0).astype(np.float32)
    p = (rng.random(shape) ** 3 * 10.0).astype(np.float32)
    z = rng.random(shape)
    h[z < 0.10] = 0.0
    p[(z > 0.05) & (z < 0.15)] = 0.0                                               # 0.05 .. 0.10: both zero
    h[(z > 0.15) & (z < 0.17)] = 1e-40
    p[(z > 0.16) & (z < 0.18)] = 3e-41
    return h, p


@pytest.mark.parametrize("shape", MASK_SHAPES)
@pytest.mark.parametrize("power", [1.0, 2.0])
def test_masks_match_float64(ops, cuda, shape, power):
    """Fewer than ten correctly rounded fp32 operations on values in [0, 1], each at most 2^-24: 1e-6 absolute."""
    h, p = mask_inputs(shape, 21)
    for mh_, mp_ in ((1.0, 1.0), (2.0, 3.0)):
        mh, mp = ops.hpss_masks(dev(h, cuda), dev(p, cuda), power, mh_, mp_)
        wh, wp = H.masks_from_medians(h, p, power, mh_, mp_)
        eh, ep = np.abs(mh.cpu().numpy() - wh).max(), np.abs(mp.cpu().numpy() - wp).max()
        print(f"masks {shape} p {power} margins ({mh_}, {mp_}): max abs err {eh:.2e}, {ep:.2e}")
        assert eh <= 1e-6 and ep <= 1e-6
        s = (mh.double() + mp.double()).cpu().numpy()
        both = (h == 0) & (p == 0)
        assert both.any()
        assert (mh.cpu().numpy()[both] == 0.5).all() and (mp.cpu().numpy()[both] == 0.5).all()
        if (mh_, mp_) == (1.0, 1.0):
            assert np.abs(s - 1.0).max() <= 1e-6
        else:
            assert s.max() <= 1.0 + 1e-6
        assert float(mh.min()) >= 0.0 and float(mh.max()) <= 1.0 and float(mp.min()) >= 0.0 and float(mp.max()) <= 1.0


def test_masks_powf(ops, cuda):
    """power 1.5 goes through powf, whose accuracy gives no derivable bound: the largest deviation from float64 was
    measured (POWF_MEASURED) and 4 times it is allowed."""
    worst = 0.0
    for shape in MASK_SHAPES:
        h, p = mask_inputs(shape, 22)
        for mh_, mp_ in ((1.0, 1.0), (2.0, 3.0)):
            mh, mp = ops.hpss_masks(dev(h, cuda), dev(p, cuda), 1.5, mh_, mp_)
            wh, wp = H.masks_from_medians(h, p, 1.5, mh_, mp_)
            worst = max(worst, np.abs(mh.cpu().numpy() - wh).max(), np.abs(mp.cpu().numpy() - wp).max())
            both = (h == 0) & (p == 0)
            assert (mh.cpu().numpy()[both] == 0.5).all() and (mp.cpu().numpy()[both] == 0.5).all()
    print(f"masks p 1.5: max abs err {worst:.3e} (measured {POWF_MEASURED:.1e}, allowed {4 * POWF_MEASURED:.1e})")
    assert worst <= 4 * POWF_MEASURED


def test_masks_options_and_errors(ops, cuda):
    from ldm_amd import _lib as L
    h, p = (dev(a, cuda) for a in mask_inputs((2, 7, 5), 23))
    mh, mp = ops.hpss_masks(h, p, 2.0, 1.0, 1.0)
    only = torch.full_like(h, -1.0)
    s = ops.stream_handle()
    L.call("ldm_hpss_masks", h.data_ptr(), p.data_ptr(), h.numel(), 2.0, 1.0, 1.0, None, only.data_ptr(), s)
    assert torch.equal(only, mp)                                                   # either output may be null
    L.call("ldm_hpss_masks", h.data_ptr(), p.data_ptr(), h.numel(), 2.0, 1.0, 1.0, only.data_ptr(), None, s)
    assert torch.equal(only, mh)
    for args, what in (((2.0, 0.5, 1.0), "margin"), ((2.0, 1.0, 0.99), "margin"), ((0.0, 1.0, 1.0), "power"),
                       ((float("inf"), 1.0, 1.0), "power"), ((float("nan"), 1.0, 1.0), "power")):
        with pytest.raises(L.LDMError, match=what):
            L.call("ldm_hpss_masks", h.data_ptr(), p.data_ptr(), h.numel(), *args, only.data_ptr(), None, s)
        with pytest.raises(ValueError, match=what):
            ops.hpss_masks(h, p, *args)
    with pytest.raises(ValueError, match="shape"):
        ops.hpss_masks(h, p[:1])


# ---- 3. the mel energy share ----------------------------------------------------------------------------------
def test_mel_share(A, ops, cuda):
    """All terms are non-negative, so each K-term sum carries a relative error of at most (K + 1) 2^-24 and the
    quotient, at most 1, an absolute one of (2K + 4) 2^-24."""
    B, F, T = 1, 1025, 9
    M, _, _, lohi, _ = A._mel_device(22050, 2048, 128, cuda)
    lh = lohi.cpu().numpy()
    assert np.array_equal(lh, H.mel_lohi(M.cpu().numpy()))
    K = int((lh[:, 1] - lh[:, 0]).max())
    rng = np.random.default_rng(31)
    P = (rng.random((B, F, T)) ** 4 * 100.0).astype(np.float32)
    P[:, :, 4] = 0.0                                                               # a silent frame
    mask = rng.random((B, F, T)).astype(np.float32)
    mask[:, ::7] = 1.0
    mask[:, 3::7] = 0.0
    Pd, md = dev(P, cuda), dev(mask, cuda)
    got = ops.mask_mel_share(Pd, md, M, lohi)
    want = H.mask_mel_share(P, mask, M.cpu().numpy())
    err = np.abs(got.cpu().numpy() - want).max()
    print(f"mel share: widest filter {K} bins, max abs err {err:.2e} (bound {(2 * K + 4) * U:.2e})")
    assert got.shape == (B, 128, T) and err <= (2 * K + 4) * U
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert bool((got[:, :, 4] == 0.5).all())
    ones = ops.mask_mel_share(Pd, torch.ones_like(md), M, lohi)
    keep = torch.ones(T, dtype=torch.bool)
    keep[4] = False
    assert bool((ones[:, :, keep] == 1.0).all()) and bool((ones[:, :, 4] == 0.5).all())
    zeros = ops.mask_mel_share(Pd, torch.zeros_like(md), M, lohi)
    assert bool((zeros[:, :, keep] == 0.0).all()) and bool((zeros[:, :, 4] == 0.5).all())
    with pytest.raises(ValueError, match="mask"):
        ops.mask_mel_share(Pd, md[:, :5], M, lohi)
    with pytest.raises(ValueError, match="lohi"):
        ops.mask_mel_share(Pd, md, M[:, :100], lohi)


# ---- 4. the separation ----------------------------------------------------------------------------------------
def test_hpss_separates_sine_from_clicks(A, ops, cuda):
    y, frames = H.sine_clicks()
    yd = dev(y, cuda)
    C, S = ops.stft(yd.unsqueeze(0), 2048, None, "both_mag")
    assert torch.equal(S, ops.stft(yd.unsqueeze(0), 2048, None, "mag"))
    mh, mp = A.hpss_masks(S[0])
    # the two masks split the spectrogram
    Cc = torch.view_as_real(C[0]).double()
    back = mh.double().unsqueeze(-1) * Cc + mp.double().unsqueeze(-1) * Cc
    rel = float((back - Cc).abs().max() / Cc.abs().max())
    print(f"mask_h C + mask_p C against C: rel {rel:.2e}")
    assert rel <= 1e-6
    h_min, p_min = H.check_sine_clicks_masks(mh.cpu().numpy(), mp.cpu().numpy(), frames)
    print(f"sine plus clicks (device): min mask_h {h_min:.6f}, min mask_p {p_min:.10f}")
    assert h_min >= 0.98
    assert p_min >= 0.99
    # and the device masks are the yardstick's on the device's own magnitudes (power 2: 1e-6, as above)
    wh, wp = H.hpss_masks(S[0].cpu().numpy())
    assert np.abs(mh.cpu().numpy() - wh).max() <= 1e-6 and np.abs(mp.cpu().numpy() - wp).max() <= 1e-6
    # the waveforms: the parts add up to the STFT round trip of y (1e-4: the round trip's own bound in test_gpu_vocoder)
    yh, yp = A.hpss(yd)
    assert yh.shape == yd.shape and yp.shape == yd.shape
    assert float((yh + yp - yd).abs().max()) <= 1e-4
    click = int(frames[2]) * H.HOP
    assert float(yp[click].abs()) > 0.5 and float(yh[click - 40:click + 40].abs().max()) < 0.75
    # the keep mask: the share of the percussive part per mel bin; the two components' shares add up to one
    kp, kh = A.hpss_keep(yd, "percussive"), A.hpss_keep(yd, "harmonic")
    assert kp.shape == (128, 1 + y.size // H.HOP) and float(kp.min()) >= 0.0 and float(kp.max()) <= 1.0
    lh = A._mel_device(22050, 2048, 128, cuda)[3].cpu().numpy()
    K = int((lh[:, 1] - lh[:, 0]).max())
    assert float((kp + kh - 1.0).abs().max()) <= 2 * (2 * K + 4) * U + 2e-6       # two shares, two masks that add to 1
    # the yardstick gives 0.99999997 above the sine at the click frames and 0.143 in the sine's mel bin between them
    assert float(kp[40:][:, torch.from_numpy(frames).to(cuda)].min()) >= 0.99     # the clicks are kept
    far, _ = H.sine_clicks_regions(kp.shape[1], frames)
    sine_mel = int(np.argmax(R.mel_filterbank(22050, 2048, 128)[:, H.sine_bin()]))
    assert float(kp[sine_mel, torch.from_numpy(far).to(cuda)].max()) <= 0.2        # the sine is not


# ---- 5. transfer_recording ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def transfer(cuda):
    import models.model as M
    from models.transfer import HOP, transfer_recording
    torch.manual_seed(0)
    model = M.LDM(32, pretrained_path="").eval().to(cuda)
    frames, overlap, T_total = 128, 32, 224                                 # two windows: [0, 128) and [96, 224)
    L = (T_total - 1) * HOP
    y = R.test_signal(L).astype(np.float32)
    y[np.arange(20, T_total - 1, 37) * HOP] += 1.0                         # a few drum hits
    content = dev(y, cuda)
    style = dev(R.test_signal(150 * HOP, variant=1), cuda)
    kw = dict(frames=frames, overlap=overlap, num_timesteps=2, n_iter=2, nnls_iters=2, seed=4)

    def run(**extra):
        return transfer_recording(model, content, style, **dict(kw, **extra))
    return run, content, T_total


def same(a, b):
    return torch.equal(a.audio, b.audio) and torch.equal(a.mel_power, b.mel_power) and \
        torch.equal(a.windows_out, b.windows_out)


def test_keep_component_is_the_keep_mask(A, transfer, cuda):
    run, content, T_total = transfer
    mask = A.hpss_keep(content, "percussive").cpu()
    assert mask.shape == (128, T_total) and 0.05 < float(mask.mean()) < 0.95
    a = run(solver="dpmpp2m", keep_component="percussive")
    b = run(solver="dpmpp2m", keep=mask)
    assert a.N == 2 and same(a, b)
    assert not same(a, run(solver="dpmpp2m"))                                # and the mask does act


def test_keep_component_unites_with_keep(A, transfer, cuda):
    from ldm_amd import longform as LF
    from models.transfer import HOP
    run, content, T_total = transfer
    span = LF.keep_mask(T_total, 128, 22050, times=[(0.0, 60 * HOP / 22050)])
    mask = A.hpss_keep(content, "harmonic", kernel_size=(17, 31), margin=(1.0, 2.0)).cpu()
    union = torch.maximum(span, mask)
    assert not torch.equal(union, span) and not torch.equal(union, mask)
    a = run(solver="dpmpp2m", keep=span, keep_component="harmonic", hpss_kernel=(17, 31), hpss_margin=(1.0, 2.0))
    assert same(a, run(solver="dpmpp2m", keep=union))


def test_no_keep_component_is_the_call_it_was(transfer):
    run, _, _ = transfer
    for solver in ("dpmpp2m", None):
        assert same(run(solver=solver, keep_component=None), run(solver=solver))
