"""Step cost of the device fingerprints: fingerprint=None / "io" / "stages" of the SAME build, timed interleaved in one process with the
method of benchmarks/ab_health.py (one model + plan + captured hipGraph per arm, shared synthetic weights and inputs, arm order rotated per
repeat, paired differences against the first arm).  ``--verify`` also exports the plan of the first arm with digests, loads it through
i2i_plan_load and times i2i_plan_verify once (wall time and the bytes digested).

    python benchmarks/ab_digest.py [--repeats 7 --steps 10 --batch 8 --size 512 --dtype bf16] [--fingerprint io stages] [--verify] [--out report.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
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
    ap.add_argument("--fingerprint", nargs="+", default=["io", "stages"], choices=["io", "stages", "all"], help="the arms beside fingerprint=None")
    ap.add_argument("--verify", action="store_true", help="export the plan with digests, load it and time i2i_plan_verify once")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from img2img_turbo_amd.arch import SD_TURBO_UNET, SD_TURBO_VAE
    from img2img_turbo_amd.digest import first_diff
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights

    dev, dtype = "cuda:0", bench.DTYPES[a.dtype]
    weights = make_pix2pix_weights(SD_TURBO_UNET, SD_TURBO_VAE, seed=1234 + 2)
    x, cap, eps, _ = bench.synth_inputs("canny", a.batch, a.size, SD_TURBO_UNET.cross_attention_dim, SD_TURBO_VAE.latent_channels, 1236)
    arms = [None] + list(a.fingerprint)
    plans, keep = [], []
    for fp in arms:
        model = Pix2Pix_Turbo(weights=weights, device=dev, dtype=dtype, fingerprint=fp)
        plan = model.get_plan(a.batch, a.size, a.size)
        model.stage(plan, x.to(dev), cap.to(dev), eps.to(dev), None)
        for _ in range(3):
            plan.replay()
        torch.cuda.synchronize()
        plans.append(plan)
        keep.append(model)
    assert all(torch.equal(plans[0].out, p.out) for p in plans[1:])
    before = [p.fingerprint() if p.fingerprint_mode else None for p in plans]
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
    for i, fp in enumerate(arms):
        m, sd = statistics.mean(ms[i]), (statistics.stdev(ms[i]) if len(ms[i]) > 1 else 0.0)
        digested = sum(nb for nb, (_o, _d, _p, label) in zip(plans[i].op_bytes, plans[i].prog.ops) if label.startswith("fingerprint: "))
        rec = {"fingerprint": fp, "ms_per_step_mean": round(m, 4), "ms_per_step_sd": round(sd, 4), "launches": len(plans[i].prog.ops),
               "taps": len(plans[i].fingerprint_labels), "digested_bytes": digested}
        if i:
            dif = [b - c for b, c in zip(ms[i], ms[0])]
            rec["paired_diff_ms_vs_none"] = round(statistics.mean(dif), 4)
            rec["paired_diff_sd"] = round(statistics.stdev(dif), 4) if len(dif) > 1 else 0.0
            rec["replays_bit_identical"] = first_diff(before[i], plans[i].fingerprint()) is None
        rep["arms"].append(rec)
        print("fingerprint=%-8s %8.3f +- %.3f ms/step  %4d launches  %3d taps  %7.1f MiB digested  %s" % (
            fp, m, sd, rec["launches"], rec["taps"], digested / 2 ** 20,
            ("diff vs None %+.3f +- %.3f ms  replays bit-identical: %s" % (rec["paired_diff_ms_vs_none"], rec["paired_diff_sd"], rec["replays_bit_identical"])) if i else ""), flush=True)
    if a.verify:
        from img2img_turbo_amd import plan_file
        lib = plans[0].lib
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "verify.i2iplan")
            t = time.perf_counter()
            info = plan_file.export_plan(plans[0], path, digests=True)
            t_export = time.perf_counter() - t
            h = lib.plan_load(path)
            t = time.perf_counter()
            rc, bad, msg = lib.plan_verify(h)
            t_verify = time.perf_counter() - t
            lib.plan_destroy(h)
        rep["verify"] = {"status": rc, "buffers": info["digests"], "bytes": info["digest_bytes"], "wall_ms": round(t_verify * 1e3, 3), "export_s": round(t_export, 2)}
        print("i2i_plan_verify: status %d, %d buffers, %.1f MiB digested, %.3f ms wall (export with digests %.1f s)"
              % (rc, info["digests"], info["digest_bytes"] / 2 ** 20, t_verify * 1e3, t_export), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rep, f, indent=1)


if __name__ == "__main__":
    main()
