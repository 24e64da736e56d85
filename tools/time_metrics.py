"""Times the transfer report on the spectrogram of a four-minute recording, P [1, 1025, 10336] and
log-mel [1, 128, 10336] (L = 10335 * 512 samples at 22050 Hz):
  * each feature kernel (ldm_onset_strength, ldm_chroma, ldm_mfcc_moments with 20 coefficients, ldm_pair_stats on two
    log-mels) beside its byte floor, one read of its inputs and one write of its outputs, at the HBM peak (8 TB/s);
  * the same four quantities computed with elementwise torch / torch.matmul on the same device: the yardstick;
  * the whole metrics.transfer_report of three four-minute waveforms (STFTs, mels, every kernel, the host read).
The inputs (42 MB and 5 MB) fit the 256 MB last-level cache, so the byte rates are cache-assisted.

Per entry: device events around the call, 3 warm-up calls, then the median and min..max of 15 calls.

Needs a HIP device.   python tools/time_metrics.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

F, T, N_MELS, N_MFCC, HOP = 1025, 10336, 128, 20, 512
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


# ---- the same quantities in torch ------------------------------------------------------------------------------
def torch_onset(db):
    return torch.clamp_min(db[:, :, 1:] - db[:, :, :-1], 0.0).mean(dim=1)


def torch_chroma(P, W):
    """W [12, F]: the filterbank as a dense matrix"""
    c = torch.matmul(W, P)
    return c / torch.linalg.vector_norm(c, dim=1, keepdim=True).clamp_min(1e-37)


def torch_mfcc_moments(db, D, w):
    c = torch.matmul(D, db.double())                       # [1, n, T]
    cw = c * w.double().unsqueeze(1)
    return w.double().sum(), cw.sum(dim=2), torch.matmul(cw, c.transpose(1, 2))


def torch_pair_stats(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    d = a - b
    return torch.stack([a.sum(), b.sum(), (a * a).sum(), (b * b).sum(), (a * b).sum(), (d * d).sum()])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_metrics: needs a HIP device")
    from ldm_amd import audio, metrics, ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    waves = [(0.1 * torch.randn((T - 1) * HOP, generator=g)).to(dev) for _ in range(3)]
    P = ops.stft(waves[0].unsqueeze(0), 2048, None, "power")
    assert tuple(P.shape) == (1, F, T)
    M, _, _, lohi, _ = audio._mel_device(22050, 2048, N_MELS, dev)
    db = 10.0 * torch.log10(ops.mel_project(P, M, lohi).clamp_min(1e-10))
    db2 = 10.0 * torch.log10(ops.mel_project(ops.stft(waves[1].unsqueeze(0), 2048, None, "power"), M, lohi).clamp_min(1e-10))
    cls, wt = metrics._chroma_device(22050, 2048, dev)
    D = metrics._dct_device(N_MFCC, N_MELS, dev)
    w = torch.ones((1, T), device=dev)
    W = torch.zeros((12, F), device=dev)
    band = cls >= 0
    idx = torch.arange(F, device=dev)[band]
    W[cls[band].long(), idx] += wt[band]
    W[(cls[band].long() + 1) % 12, idx] += 1.0 - wt[band]
    E = 1 + N_MFCC + N_MFCC * (N_MFCC + 1) // 2
    res = {"F": F, "T": T, "n_mels": N_MELS, "n_mfcc": N_MFCC, "warmup": WARMUP, "runs": RUNS, "entries": {}}

    def report(key, r, nbytes=None):
        if nbytes is not None:
            r["floor_bytes"] = nbytes
            r["floor_us"] = nbytes / HBM_PEAK * 1e6
            r["fraction_of_hbm_peak"] = nbytes / (r["median_ms"] * 1e-3) / HBM_PEAK
        res["entries"][key] = r
        extra = "" if nbytes is None else (f"; floor {nbytes / 1e6:.1f} MB = {r['floor_us']:.2f} us at 8 TB/s, "
                                           f"{100 * r['fraction_of_hbm_peak']:.2f} % of the HBM peak")
        print(f"{key}: {r['median_ms']:.3f} ms (min {r['min']:.3f}, max {r['max']:.3f}; {RUNS} calls){extra}", flush=True)

    report("ldm_onset_strength", measure(lambda: ops.onset_strength(db, 1)), (N_MELS * T + T) * 4)
    report("torch onset", measure(lambda: torch_onset(db)))
    report("ldm_chroma", measure(lambda: ops.chroma(P, cls, wt)), (F * T + 12 * T) * 4)
    report("torch chroma (matmul)", measure(lambda: torch_chroma(P, W)))
    report("ldm_mfcc_moments", measure(lambda: ops.mfcc_moments(db, D, w)), (N_MELS * T + T) * 4 + E * 8)
    report("torch mfcc moments (float64 matmul)", measure(lambda: torch_mfcc_moments(db, D, w)))
    report("ldm_pair_stats", measure(lambda: ops.pair_stats(db.reshape(1, -1), db2.reshape(1, -1))), 2 * N_MELS * T * 4)
    report("torch pair sums (float64)", measure(lambda: torch_pair_stats(db, db2)))
    report("transfer_report (whole call, three waveforms)",
           measure(lambda: metrics.transfer_report(waves[0], waves[1], waves[2])))
    # the torch forms compute what the kernels compute
    env = ops.onset_strength(db, 1)
    res["onset_max_abs_diff"] = float((env[:, 1:] - torch_onset(db)).abs().max())
    res["chroma_max_abs_diff"] = float((ops.chroma(P, cls, wt) - torch_chroma(P, W)).abs().max())
    mom = ops.mfcc_moments(db, D, w)[0]
    res["mfcc_mean_max_rel_diff"] = float(((mom[1:1 + N_MFCC] - torch_mfcc_moments(db, D, w)[1][0]).abs()
                                           / mom[1:1 + N_MFCC].abs().clamp_min(1e-300)).max())
    print(f"kernel against torch: onset {res['onset_max_abs_diff']:.2e}, chroma {res['chroma_max_abs_diff']:.2e}, "
          f"mfcc sums rel {res['mfcc_mean_max_rel_diff']:.2e}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
