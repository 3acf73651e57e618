"""Step cost of the numerical health scans: health=None / "stages" / "all" of the SAME build, timed interleaved in one process with the
method of benchmarks/ab.py (one model + plan + captured hipGraph per arm, shared synthetic weights and inputs, arm order rotated per
repeat, paired differences against the first arm).  ``--per-image`` adds the per-image twin of every health arm (health_per_image=True:
one record per tap and image, the CLEAR op in front and the JUDGE op behind), so its step cost reads beside the whole-batch form.

    python benchmarks/ab_health.py [--repeats 7 --steps 10 --batch 8 --size 512 --dtype bf16] [--per-image] [--health stages all] [--out report.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--per-image", action="store_true", help="also time every health arm with health_per_image=True")
    ap.add_argument("--health", nargs="+", default=["stages", "all"], choices=["stages", "all"], help="the health arms (beside health=None)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from img2img_turbo_amd.arch import SD_TURBO_UNET, SD_TURBO_VAE
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights

    dev, dtype = "cuda:0", bench.DTYPES[a.dtype]
    weights = make_pix2pix_weights(SD_TURBO_UNET, SD_TURBO_VAE, seed=1234 + 2)
    x, cap, eps, _ = bench.synth_inputs("canny", a.batch, a.size, SD_TURBO_UNET.cross_attention_dim, SD_TURBO_VAE.latent_channels, 1236)
    arms = [(None, False)] + [(h, per) for h in a.health for per in ((False, True) if a.per_image else (False,))]
    plans, keep = [], []
    for health, per_image in arms:
        model = Pix2Pix_Turbo(weights=weights, device=dev, dtype=dtype, health=health, health_per_image=per_image)
        plan = model.get_plan(a.batch, a.size, a.size)
        model.stage(plan, x.to(dev), cap.to(dev), eps.to(dev), None)
        for _ in range(3):
            plan.replay()
        torch.cuda.synchronize()
        plans.append(plan)
        keep.append(model)
    assert all(torch.equal(plans[0].out, p.out) for p in plans[1:])
    ms = [[] for _ in plans]
    for r in range(a.repeats):
        order = list(range(len(plans)))
        order = order[r % len(order):] + order[:r % len(order)]
        for i in order:
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(a.steps):
                plans[i].replay()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t) / a.steps * 1e3)
    rep = {"batch": a.batch, "size": a.size, "dtype": a.dtype, "repeats": a.repeats, "steps_per_repeat": a.steps, "arms": []}
    for i, (health, per_image) in enumerate(arms):
        m, sd = statistics.mean(ms[i]), (statistics.stdev(ms[i]) if len(ms[i]) > 1 else 0.0)
        scanned = sum(r_ * c_ * t.element_size() for t, r_, c_, _ in plans[i].health_taps)
        rec = {"health": health, "per_image": per_image, "ms_per_step_mean": round(m, 4), "ms_per_step_sd": round(sd, 4), "launches": len(plans[i].prog.ops),
               "taps": len(plans[i].health_labels), "scanned_bytes": scanned}
        if i:
            dif = [b - c for b, c in zip(ms[i], ms[0])]
            rec["paired_diff_ms_vs_none"] = round(statistics.mean(dif), 4)
            rec["paired_diff_sd"] = round(statistics.stdev(dif), 4) if len(dif) > 1 else 0.0
            bad = plans[i].health_first_bad()
            rec["first_bad"] = bad and bad["label"]
            if per_image:
                rec["bad_images"] = [v["image"] for v in plans[i].health_verdict() if v["first_bad"]]
        rep["arms"].append(rec)
        print("health=%-18s %8.3f +- %.3f ms/step  %4d launches  %3d taps  %6.1f MiB scanned  %s" % (
            "%s%s" % (health, " per image" if per_image else ""), m, sd, rec["launches"], rec["taps"], scanned / 2 ** 20,
            ("diff vs None %+.3f +- %.3f ms" % (rec["paired_diff_ms_vs_none"], rec["paired_diff_sd"])) if i else ""), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
