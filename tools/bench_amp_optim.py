"""Time one AMP optimizer step -- non-finite check + Adam update + step-counter finish, the three launches of
``climategan_amd.optim.GradScaler.step`` -- on the real parameter shape lists of G (105.4 M parameters) and D (26.5 M) of
the default configuration, against torch's own path on the same GPU.  Prints one JSON line.

    python tools/bench_amp_optim.py [--window-ms 300] [--warmup 3] [--repeats 5]

Per model (median of ``--repeats`` event-timed windows, each of as many steps as fill about ``--window-ms`` of device
time, the two variants alternating; the spread is the min and max of those windows):
  hip_ms      ``GradScaler.step(Adam) + update()`` of this package, steps back to back: check -> update -> finish.  Back to
              back, each step resolves the flag of the one before it, so this is max(host, device) per step
  hip_device_ms   one step's three launches queued behind other device work (the host's table building is over before the
              device gets to them): the device time alone
  torch_ms    the yardstick: ``torch.amp.GradScaler.step(torch.optim.Adam) + update()`` on clones of the same tensors
              (``fused=True`` where this torch accepts it on the device, else the foreach implementation; reported in
              ``torch_impl``).  torch's ``step`` reads the non-finite flag back on the host.
  hip_gbps    the algorithmic bytes -- 4 B per element for the check, 16 B read + 12 B written for the update -- over
              hip_device_ms; ``share_of_stream_rate``: against the 5.5 TB/s the repository's streaming kernels reach.
  hip_host_ms the host time of ``step() + update()`` with NO synchronisation around it (wall clock over a window that ends
              before the device does): what the host pays to enqueue a step; the launches do not wait.
Before anything is timed both variants take three steps on the same gradients and must agree to 2e-6 (the bound of
tests/test_gpu_amp_optim.py) or the tool exits with status 1 and prints no timing.
"""
import argparse
import json
import math
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from climategan_amd.config import default_opts  # noqa: E402
from climategan_amd.optim import Adam, GradScaler  # noqa: E402

STREAM_TBPS = 5.5
BYTES_PER_ELEMENT = 4 + 16 + 12


def model_shapes():
    """Trainable parameter shapes of the default G and D, built on the host (no weights are needed)."""
    from climategan_amd.discriminator import create_discriminator
    from climategan_amd.generator import create_generator

    opts = default_opts()
    G = create_generator(opts, device="cpu", no_init=True)
    D = create_discriminator(opts, "cpu")
    return {"G": [tuple(p.shape) for p in G.parameters() if p.requires_grad],
            "D": [tuple(p.shape) for n, p in D.named_parameters() if not n.endswith(("weight_u", "weight_v"))]}


def window_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def torch_adam(params, **kw):
    try:
        opt = torch.optim.Adam(params, fused=True, **kw)
        return opt, "fused"
    except Exception:
        return torch.optim.Adam(params, foreach=True, **kw), "foreach"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=300.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    result = {"what": "AMP optimizer step (check + Adam + finish) on the default G / D parameter lists",
              "device": torch.cuda.get_device_name(0), "window_ms": args.window_ms, "repeats": args.repeats, "models": {}}
    kw = dict(lr=5e-5, betas=(0.5, 0.999))
    busy = torch.randn(8192, 8192, device="cuda", dtype=torch.bfloat16)
    for name, shapes in model_shapes().items():
        g = torch.Generator(device="cuda").manual_seed(0)
        mine = [torch.nn.Parameter(torch.randn(s, device="cuda", generator=g) * 0.05) for s in shapes]
        theirs = [torch.nn.Parameter(p.detach().clone()) for p in mine]
        numel = sum(p.numel() for p in mine)
        scale = 1024.0
        for a, b in zip(mine, theirs):
            a.grad = torch.randn(a.shape, device="cuda", generator=g) * 1e-2 * scale
            b.grad = a.grad.clone()
        opt, scaler = Adam(mine, **kw), GradScaler(init_scale=scale, growth_interval=10 ** 9)
        ref, impl = torch_adam(theirs, **kw)
        ref_scaler = torch.amp.GradScaler("cuda", init_scale=scale, growth_interval=10 ** 9)
        ref_scaler.scale(torch.zeros((), device="cuda"))
        grads = [b.grad.clone() for b in theirs]

        def hip_step():
            scaler.step(opt)
            scaler.update()

        def torch_step_fresh():
            torch._foreach_copy_([b.grad for b in theirs], keep)
            ref_scaler.step(ref)
            ref_scaler.update()

        keep = [gr.clone() for gr in grads]
        for b, gr in zip(theirs, grads):
            b.grad = gr
        for _ in range(3):                          # agreement first, on identical scaled gradients
            hip_step()
            torch_step_fresh()
        worst = max(((a.detach() - b.detach()).abs().max() / max(1.0, b.detach().abs().max().item())).item()
                    for a, b in zip(mine, theirs))
        if not worst <= 2e-6:
            sys.exit("bench_amp_optim: the HIP and the torch step disagree on %s (max relative diff %.3g): nothing timed"
                     % (name, worst))
        # torch's yardstick includes restoring the scaled gradients (its unscale is in place, so a second step on the same
        # tensors would see unscaled values): the restore is timed on its own and subtracted
        variants = {"hip": hip_step, "torch": torch_step_fresh,
                    "restore": lambda: torch._foreach_copy_([b.grad for b in theirs], keep)}
        for fn in variants.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        iters = {k: max(10, math.ceil(args.window_ms / window_ms(fn, 10))) for k, fn in variants.items()}
        times = {k: [] for k in variants}
        for _ in range(args.repeats):
            for k, fn in variants.items():
                times[k].append(window_ms(fn, iters[k]))
        med = {k: statistics.median(v) for k, v in times.items()}
        torch_ms = med["torch"] - med["restore"]
        host, dev = [], []
        for _ in range(2 * args.repeats):
            # host time to ENQUEUE one step: the previous step's flag is resolved first (in the trainer the other model's
            # whole update lies in between), the clock stops before the device is waited for
            scaler.get_scale()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hip_step()
            host.append((time.perf_counter() - t0) * 1e3)
            # device time of the three launches: queued behind ~10 ms of other work, so that the host's table building
            # is over before the device gets to them
            scaler.get_scale()
            torch.cuda.synchronize()
            for _ in range(6):
                torch.mm(busy, busy)
            dev.append(window_ms(hip_step, 1))
        torch.cuda.synchronize()
        nbytes = numel * BYTES_PER_ELEMENT
        dev_ms = statistics.median(dev)
        result["models"][name] = {
            "tensors": len(shapes), "parameters": numel, "hip_ms": med["hip"], "hip_min_max": [min(times["hip"]), max(times["hip"])],
            "torch_impl": impl, "torch_ms": torch_ms, "torch_with_restore_ms": med["torch"],
            "torch_with_restore_min_max": [min(times["torch"]), max(times["torch"])], "restore_ms": med["restore"],
            "torch_over_hip": torch_ms / med["hip"], "steps_per_window": iters, "algorithmic_bytes": nbytes,
            "hip_device_ms": dev_ms, "hip_device_min_max": [min(dev), max(dev)],
            "hip_gbps": nbytes / (dev_ms * 1e6), "share_of_stream_rate": nbytes / (dev_ms * 1e6) / (STREAM_TBPS * 1e3),
            "hip_host_ms": statistics.median(host), "hip_host_min_max": [min(host), max(host)],
            "max_rel_diff_hip_vs_torch": worst, "skipped_steps": scaler.skipped_steps}
        del mine, theirs, opt, ref, grads, keep
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
