"""Times the harmonic / percussive separation on the spectrogram of a four-minute recording,
[1, 1025, 10336] (L = 10335 * 512 samples at 22050 Hz), window 31:
  * the two median passes alone (ldm_median_filter along time and along frequency), each beside its byte floor, one
    read and one write of F T floats, as a fraction of the HBM peak (8 TB/s);
  * ldm_hpss_masks (power 2) and ldm_mask_mel_share;
  * the whole audio.hpss_keep of the waveform (two STFTs, two medians, the masks, the share).
The 42 MB spectrogram fits the 256 MB last-level cache, so the byte figures are cache-assisted; the medians are bound
by their compares, not by bytes.  Also prints the largest deviation of the power-1.5 masks (powf) from float64 on the
inputs of tests/test_gpu_hpss.py.

Per entry: device events around the call, 3 warm-up calls, then the median and min..max of 15 calls.

Needs a HIP device.   python tools/time_hpss.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd"), os.path.join(ROOT, "tests")]

F, T, WIN, HOP = 1025, 10336, 31, 512
WARMUP, RUNS = 3, 15
HBM_PEAK = 8.0e12


def measure(fn):
    ts = []
    for i in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ts.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ts), "min": min(ts), "max": max(ts)}


def powf_deviation(dev):
    import hpss_ref as H
    import test_gpu_hpss as G
    from ldm_amd import ops
    worst = 0.0
    for shape in G.MASK_SHAPES:
        h, p = G.mask_inputs(shape, 22)
        for mh_, mp_ in ((1.0, 1.0), (2.0, 3.0)):
            mh, mp = ops.hpss_masks(torch.from_numpy(h).to(dev), torch.from_numpy(p).to(dev), 1.5, mh_, mp_)
            wh, wp = H.masks_from_medians(h, p, 1.5, mh_, mp_)
            worst = max(worst, float(np.abs(mh.cpu().numpy() - wh).max()), float(np.abs(mp.cpu().numpy() - wp).max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_hpss: needs a HIP device")
    from ldm_amd import audio, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    y = (0.1 * torch.randn((T - 1) * HOP, generator=g)).to(dev)
    S = ops.stft(y.unsqueeze(0), 2048, None, "mag")
    P = ops.stft(y.unsqueeze(0), 2048, None, "power")
    assert tuple(S.shape) == (1, F, T)
    M, _, _, lohi, _ = audio._mel_device(22050, 2048, 128, dev)
    out = torch.empty_like(S)
    harm, perc = ops.median_filter(S, WIN, 1), ops.median_filter(S, WIN, 0)
    mh, mp = ops.hpss_masks(harm, perc, 2.0, 1.0, 1.0)
    floor = 2 * F * T * 4
    res = {"F": F, "T": T, "win": WIN, "warmup": WARMUP, "runs": RUNS, "median_pass_floor_bytes": floor, "entries": {}}

    def report(key, r, nbytes=None):
        if nbytes is not None:
            r["bytes"] = nbytes
            r["TB_per_s"] = nbytes / (r["median_ms"] * 1e-3) / 1e12
            r["fraction_of_hbm_peak"] = nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK
        res["entries"][key] = r
        extra = "" if nbytes is None else (f"; {nbytes / 1e6:.1f} MB, {r['TB_per_s']:.3f} TB/s, "
                                           f"{100 * r['fraction_of_hbm_peak']:.2f} % of the HBM peak")
        print(f"{key}: {r['median_ms']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}; {RUNS} calls){extra}", flush=True)

    report("median along time (harmonic)", measure(lambda: ops.median_filter(S, WIN, 1, out=out)), floor)
    report("median along frequency (percussive)", measure(lambda: ops.median_filter(S, WIN, 0, out=out)), floor)
    report("hpss_masks p=2", measure(lambda: ops.hpss_masks(harm, perc, 2.0, 1.0, 1.0)), 4 * F * T * 4)
    report("mask_mel_share", measure(lambda: ops.mask_mel_share(P, mp, M, lohi)))
    report("stft (magnitude)", measure(lambda: ops.stft(y.unsqueeze(0), 2048, None, "mag")))
    report("hpss_keep (whole call)", measure(lambda: audio.hpss_keep(y, "percussive")))
    res["powf_max_abs_deviation_p1.5"] = powf_deviation(dev)
    print(f"masks at power 1.5: max abs deviation from float64 {res['powf_max_abs_deviation_p1.5']:.3e}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
