"""Times what style guidance costs the reverse loop: the captured 49-iteration loop (linspace(99, 0,
50): the flagship's) on the 16 x 64 latent, fp32 and fp16 operands, DDIM and 2M update, for
  * the guided loop at B = 4 (the body runs at batch 8: targets, then bases), scale 2.5,
  * the plain loop at B = 8 (what the body costs without the second dec1 launch and the duplicated state), and
  * the plain loop at B = 4 (what a user pays today for the same four samples).

Per configuration: one GraphedDDIM, 3 warm-up replays, then the median and the min..max of 15 replays between stream
events, divided by the iteration count.  The loop's pre-loop work (time MLP, K/V projections, key fold) is inside.

Needs a HIP device.   python tools/time_guidance.py [--json out]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "music-style-transfer-ldm_amd")]

H, W, ITERS = 16, 64, 49
WARMUP, RUNS = 3, 15


def build(dev, dtype, B, solver, guided):
    import models.model as M
    from ldm_amd.engine import GraphedDDIM, UNetEngine
    torch.manual_seed(0)
    ldm = M.LDM(32, pretrained_path="").eval().to(dev)
    eng = UNetEngine(ldm.unet, dtype=dtype)
    g = torch.Generator().manual_seed(B)
    z = torch.randn(B, 32, H, W, generator=g).to(dev)
    maps = [torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev), torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev),
            torch.rand(B, 256, H // 4, W // 4, generator=g).to(dev), torch.rand(B, 512, H // 8, W // 8, generator=g).to(dev)]
    times = torch.linspace(99, 0, ITERS + 1).long()
    fd = ldm.noise_scheduler
    coef = (fd.multistep_coefs(times) if solver == "msolver" else fd.reverse_coefs(times)).to(dev)
    t_table = times[:-1].view(ITERS, 1).expand(ITERS, B).contiguous().to(dev)
    kw = dict(base=(maps[2], maps[3], None, None), guidance_scale=2.5) if guided else {}
    with torch.no_grad():
        return GraphedDDIM(eng, z, maps[0], maps[1], t_table, coef, 0.0, logs=solver == "msolver", solver=solver, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None, help="also write the numbers to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_guidance: needs a HIP device")
    dev = torch.device("cuda:0")
    res = {"H": H, "W": W, "iterations": ITERS, "warmup": WARMUP, "runs": RUNS, "loops": {}}
    for dtype in ("fp32", "fp16"):
        for solver in ("ddim", "msolver"):
            for name, B, guided in (("guided-B4", 4, True), ("plain-B8", 8, False), ("plain-B4", 4, False)):
                gd = build(dev, dtype, B, solver, guided)
                ts = []
                for i in range(WARMUP + RUNS):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    gd.replay()
                    b.record()
                    b.synchronize()
                    if i >= WARMUP:
                        ts.append(a.elapsed_time(b) * 1e3 / ITERS)
                assert bool(torch.isfinite(gd.x).all())
                r = {"median_us_per_iteration": statistics.median(ts), "min": min(ts), "max": max(ts)}
                res["loops"][f"{dtype}-{solver}-{name}"] = r
                print(f"{dtype} {solver} {name}: {r['median_us_per_iteration']:.1f} us per iteration (min {r['min']:.1f}, "
                      f"max {r['max']:.1f}; {RUNS} replays of the {ITERS}-iteration graph)", flush=True)
                del gd
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
