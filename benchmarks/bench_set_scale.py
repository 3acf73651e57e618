"""Cost of moving the LoRA scale r: Packer.set_scale on full SD-Turbo-size synthetic weights (bf16), per layer (one i2i_lora_merge launch
per adapted layer + the host TwinConv fold: the default path) against the scale program (live_scale: one grouped launch, the
LayerNorm-fold layers, the TwinConv fold kernel), on one device in one process, interleaved.

    python benchmarks/bench_set_scale.py [--rounds 30] [--warmup 5]

Each sample is one set_scale between two values of r for the UNet and the VAE packer together, timed on the host from call to
synchronised completion (what a slider frame waits for) and, for the device part alone, with an event pair.  The two paths alternate
sample by sample (A B A B ...), so drift and clock state hit both alike; reported are the median and the 10th / 90th percentile of each, the
median of the paired differences, the bytes the merge moves (fp32 masters and LoRA factors read, 16-bit weights written) and what
fraction of a 6.3 TB/s copy rate the grouped path reaches.  One JSON line at the end."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_RATE = 6.3e12      # bytes / s a device copy reaches on an MI355X


def merge_bytes(pk):
    rd = wr = 0
    for p, _ in pk._merges:
        rd += 4 * p.N * p.K + 4 * p.rank * (p.K + p.N)
        wr += torch.empty(0, dtype=pk.dtype).element_size() * p.N * p.K
    return rd, wr


def pct(v, q):
    s = sorted(v)
    return s[min(len(s) - 1, int(q * len(s)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--arch", default="sd-turbo", choices=["sd-turbo", "tiny"])
    a = ap.parse_args()
    from img2img_turbo_amd import arch
    from img2img_turbo_amd.pix2pix_turbo import Pix2Pix_Turbo
    from img2img_turbo_amd.synth import make_pix2pix_weights
    ua, va = (arch.TINY_UNET, arch.TINY_VAE) if a.arch == "tiny" else (arch.SD_TURBO_UNET, arch.SD_TURBO_VAE)
    w = make_pix2pix_weights(ua, va, seed=1234, sketch=True)
    models = {}
    for name, live in (("per_layer", False), ("grouped", True)):
        m = Pix2Pix_Turbo(weights=w, device="cuda:0", dtype=torch.bfloat16, live_scale=live)
        m.get_plan(1, 512 if a.arch != "tiny" else 64, 512 if a.arch != "tiny" else 64, stochastic=True, r=0.4)      # packs every layer the forward uses
        models[name] = m
    torch.cuda.synchronize()
    g = models["grouped"]
    layers = sum(len(pk._merges) for pk in g._packers.values())
    grouped = sum(pk.scale_program().n_grouped for pk in g._packers.values())
    rd, wr = map(sum, zip(*(merge_bytes(pk) for pk in g._packers.values())))
    host = {k: [] for k in models}
    devt = {k: [] for k in models}
    rs = (0.4, 0.8)
    for i in range(a.warmup + a.rounds):
        r = rs[(i + 1) % 2]
        for name, m in models.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            m.set_lora_scale(r)
            e1.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if i >= a.warmup:
                host[name].append((t1 - t0) * 1e3)
                devt[name].append(e0.elapsed_time(e1))
    out = {"bench": "set_scale", "arch": a.arch, "dtype": "bf16", "rounds": a.rounds, "adapted_layers": layers, "grouped_layers": grouped,
           "launches_per_layer_path": layers, "launches_grouped_path": sum(len(pk.scale_program().groups) + pk.scale_program().prog.n for pk in g._packers.values()),
           "bytes_read": rd, "bytes_written": wr, "ideal_ms_at_6.3TBps": (rd + wr) / COPY_RATE * 1e3}
    for name in models:
        for kind, v in (("host_ms", host[name]), ("device_ms", devt[name])):
            out["%s_%s" % (name, kind)] = {"median": pct(v, 0.5), "p10": pct(v, 0.1), "p90": pct(v, 0.9)}
    diff = [p - q for p, q in zip(host["per_layer"], host["grouped"])]
    out["paired_host_diff_ms"] = {"median": pct(diff, 0.5), "p10": pct(diff, 0.1), "p90": pct(diff, 0.9)}
    out["grouped_fraction_of_copy_rate"] = out["ideal_ms_at_6.3TBps"] / out["grouped_device_ms"]["median"]
    for k, v in out.items():
        print("%-28s %s" % (k, v))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
