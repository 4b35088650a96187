"""Times of the prediction path on one GPU, recorded and not gated:

  * ``mart_topk`` (Fn.topk) against ``torch.topk`` and ``torch.sort`` on the SAME device tensor: [128, 2063], [128, 11292], [256, 11292],
    [128, 42007] at k = 10 and k = 64 -- device events around each launch, the three contenders interleaved in one process, medians;
  * ``predict_step`` against ``validation_step`` on the same 128-example batch (bench.py's model and batch), both evaluation precisions -- a host
    clock around calls that end in the copy of the result to the host.

The shader clock the box granted during the timed region (median of rocm-smi samples, bench.PowerSampler) rides along.  Prints one JSON line;
``--out`` also writes it.

    python tools/bench_topk.py [--iters 200] [--warmup 20] [--steps 10] [--out profiles/r10_topk.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(128, 2063), (128, 11292), (256, 11292), (128, 42007)]
KS = [10, 64]


def _median(v):
    return sorted(v)[len(v) // 2]


def kernel_times(iters: int, warmup: int) -> list:
    from mkg_analogy_amd import functional as Fn
    rows = []
    for R, C in SIZES:
        x = torch.randn((R, C), device="cuda", generator=torch.Generator(device="cuda").manual_seed(R + C))
        for k in KS:
            contenders = {"mart_topk": lambda: Fn.topk(x, k), "torch_topk": lambda: torch.topk(x, k, dim=1, largest=True, sorted=True),
                          "torch_sort": lambda: torch.sort(x, dim=1, descending=True, stable=True)}
            times = {n: [] for n in contenders}
            for it in range(warmup + iters):
                for name, fn in contenders.items():                        # interleaved: a clock change hits all three alike
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    if it >= warmup:
                        times[name].append(a.elapsed_time(b) * 1e3)
            same = bool(torch.equal(Fn.topk(x, k)[1], torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]))
            rows.append({"R": R, "C": C, "k": k, "mb_read_once": round(R * C * 4 / 1e6, 2), "indices_equal_stable_sort": same,
                         **{f"{n}_us_median": round(_median(t), 2) for n, t in times.items()},
                         **{f"{n}_us_min": round(min(t), 2) for n, t in times.items()}})
    return rows


def step_times(steps: int, warmup: int) -> list:
    import bench
    from mkg_analogy_amd import data_synth as D
    dev = torch.device("cuda", 0)
    model, lit, cfg = bench.build(16, seed=0, device=dev, backbone="mkgformer")
    model.eval()
    batch = D.make_batch(128, 64, seed=1234, device=dev)
    out = []
    for prec in ("fp32", "bf16"):
        lit.args.eval_precision = prec
        hooks = {"validation_step": lambda: lit.validation_step(dict(batch), 0), "predict_step_k10": lambda: lit.predict_step(dict(batch), 0, k=10)}
        times = {n: [] for n in hooks}
        for it in range(warmup + steps):
            for name, fn in hooks.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()                                                        # ends in the copy of its arrays to the host
                torch.cuda.synchronize()
                if it >= warmup:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        out.append({"eval_precision": prec, "B": 128, "L": 64, **{f"{n}_ms_median": round(_median(t), 3) for n, t in times.items()}})
    lit.args.pop("eval_precision")
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk needs the GPU: a time taken elsewhere says nothing")
    import bench
    with bench.PowerSampler(0) as ps:
        kern = kernel_times(a.iters, a.warmup)
        steps = step_times(a.steps, max(2, a.warmup // 10))
    power_w, sclk_mhz, n = ps.median()
    res = {"tool": "tools/bench_topk.py", "device": torch.cuda.get_device_name(0), "iters": a.iters, "sclk_mhz_median": sclk_mhz, "power_w_median": power_w,
           "clock_samples": n, "timing": "kernels: device events per launch, contenders interleaved, medians (us); hooks: host clock around calls "
           "that end in the device-to-host copy of the result (ms)", "kernels": kern, "hooks": steps}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
