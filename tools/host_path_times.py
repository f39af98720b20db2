#!/usr/bin/env python3
"""Host time of the resident batch's step outside the kernel: (a) the wall time of the ctx.enqueue(...) call on an idle stream
(validation, launch planning, the launch itself), (b) the wall time of ctx.get_poses() after a ctx.synchronize() (staging copy,
unpack, the numpy arrays).  The batch is bench.py's default resident batch, built by bench.py's own build_batch.  One JSON line;
medians over --steps steps.

    python tools/host_path_times.py [--batch N] [--steps K]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=40000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    own = ap.parse_args()
    if own.steps < 20:
        ap.error("--steps must be at least 20")
    sys.argv = [os.path.join(ROOT, "bench.py"), "--batch", str(own.batch)]
    import bench                                    # imports torch before the HIP library (one HIP runtime per process)
    import torch
    from rgbd_odometry_amd import DvoContext
    from rgbd_odometry_amd.capi import DVO_FLAG_FINAL_OUTPUTS, DVO_FLAG_IDENTITY_START
    args = bench.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("host_path_times.py needs a HIP device")
    bench.keep_host_memory_mapped()
    iters = [args.iters] * args.levels
    flags = DVO_FLAG_IDENTITY_START | DVO_FLAG_FINAL_OUTPUTS
    ctx = DvoContext(args.batch)
    bench.build_batch(ctx, args, 0)
    stream = torch.cuda.Stream()
    ctx.set_stream(stream.cuda_stream)
    t_enq, t_get, t_step = [], [], []
    for k in range(own.warmup + own.steps):
        ctx.synchronize()                           # (a) starts on an idle stream
        t0 = time.perf_counter()
        ctx.enqueue(iters, flags=flags)
        t1 = time.perf_counter()
        ctx.synchronize()                           # (b) holds no kernel time
        t2 = time.perf_counter()
        ctx.get_poses()
        t3 = time.perf_counter()
        if k >= own.warmup:
            t_enq.append(t1 - t0); t_get.append(t3 - t2); t_step.append(t3 - t0)
    out = {"tool": "host_path_times", "batch": args.batch, "steps": own.steps, "memo": os.environ.get("DVO_LAUNCH_MEMO", ""),
           "enqueue_ms_median": 1e3 * statistics.median(t_enq), "enqueue_ms_min": 1e3 * min(t_enq), "enqueue_ms_max": 1e3 * max(t_enq),
           "get_poses_ms_median": 1e3 * statistics.median(t_get), "get_poses_ms_min": 1e3 * min(t_get), "get_poses_ms_max": 1e3 * max(t_get),
           "step_ms_median": 1e3 * statistics.median(t_step)}
    if hasattr(ctx, "enqueue_counts"):
        out["enqueue_counts"] = list(ctx.enqueue_counts())
    print(json.dumps(out))


if __name__ == "__main__":
    main()
