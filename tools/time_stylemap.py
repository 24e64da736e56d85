"""Times what the style map costs the reverse loop: the captured 10-step 2M loop (sample_times(99, 10))
on the 16 x 64 latent at B = 8 with R = 2 stacked references, fp32 operands, for
  * the key-bias mix (weights per reference and sample, folded into bf by the prepare phase),
  * the style map (reference biases per query position, read by every step's two attentions),
  * the style map rewritten by GraphedDDIM.set_style_map before every replay (a new map per window of a recording):
    the host-side value check, the two copies into the static buffers and the replay, and no prepare launch.

Per configuration: one captured graph, 3 warm-up replays, then the median and the min..max of 15 replays between stream
events.  Each loop's first replay launches its prepare graph; the timed replays do not (prepare_launches is printed).

Needs a HIP device.   python tools/time_stylemap.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

B, H, W, R, STEPS = 8, 16, 64, 2, 10
WARMUP, RUNS = 3, 15


def build(dev, form):
    import models.model as M
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    eng = UNetEngine(ldm.unet)
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, 32, H, W, generator=g).to(dev)
    s5 = torch.rand(B, 256, R * H // 4, W // 4, generator=g).to(dev)
    s6 = torch.rand(B, 512, R * H // 8, W // 8, generator=g).to(dev)
    times = ldm.sample_times(99, STEPS)
    coef = ldm.noise_scheduler.multistep_coefs(times).to(dev)
    t_table = times[:-1].view(STEPS, 1).expand(STEPS, B).contiguous().to(dev)
    maps = [M.LDM.style_map_bias(torch.rand(B, R, H, W, generator=g) + 0.05, H, W) for _ in range(2)]
    maps = [(a.to(dev), b.to(dev)) for a, b in maps]
    kw = {}
    if form == "mix":
        lw = torch.log(torch.rand(B, R, generator=g) + 0.05)
        kw = dict(key_bias5=lw.repeat_interleave(H * W // 16, dim=1).contiguous().to(dev),
                  key_bias6=lw.repeat_interleave(H * W // 64, dim=1).contiguous().to(dev))
    else:
        kw = dict(ref_bias5=maps[0][0], ref_bias6=maps[0][1])
    with torch.no_grad():
        gd = GraphedDDIM(eng, z, s5, s6, t_table, coef, 0.0, logs=True, solver="msolver", **kw)
    return gd, maps


def measure(gd, maps=None):
    ts = []
    for i in range(WARMUP + RUNS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if maps is not None:
            gd.set_style_map(*maps[i % 2])
        gd.replay()
        b.record()
        b.synchronize()
        if i >= WARMUP:
            ts.append(a.elapsed_time(b) * 1e3)
    assert bool(torch.isfinite(gd.x).all())
    return {"median_us_per_loop": statistics.median(ts), "min": min(ts), "max": max(ts),
            "prepare_launches": gd.prepare_launches}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_stylemap: needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"B": B, "H": H, "W": W, "R": R, "steps": STEPS, "warmup": WARMUP, "runs": RUNS, "loops": {}}
    for name, form, rewrite in (("key-bias-mix", "mix", False), ("style-map", "map", False),
                                ("style-map-rewritten", "map", True)):
        gd, maps = build(dev, form)
        r = measure(gd, maps if rewrite else None)
        res["loops"][name] = r
        print(f"{name}: {r['median_us_per_loop']:.1f} us per {STEPS}-step loop (min {r['min']:.1f}, max {r['max']:.1f}; "
              f"{RUNS} replays; prepare launches {r['prepare_launches']})", flush=True)
        del gd
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
