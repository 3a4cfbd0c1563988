"""What tools/bench_{fps,knn,normals,voxel,icp,fpfh,ransac}.py share: the HIP-event timer, the checks before a measurement, the raw-call plumbing, and
the harness of those that run one child process per shape under a time limit and stop at the first failure."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, reps, inner=1):
    """`fn` warmed up once, then the median over `reps` windows of HIP-event time per call; a window holds `inner` calls enqueued back to
    back (kernels of tens of microseconds: one launch is below what an event pair resolves)"""
    import torch
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return statistics.median(ms)


def setup(script):
    """refuse a CPU run, build the library, return gecco_amd.pointops"""
    import torch
    if not torch.cuda.is_available():
        raise SystemExit(f"{os.path.basename(script)} needs a GPU: a CPU run says nothing about these kernels")
    import __graft_entry__ as ge
    ge.build()
    from gecco_amd import pointops
    return pointops


def vp(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def emit(bench, res, out):
    import torch
    line = json.dumps({"bench": bench, "device": torch.cuda.get_device_name(0), **res})
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main(script, bench, shapes, step_seconds, run_shape, reps=10, options=()):
    """`script [--reps R] [--out FILE]` plus `options`, (flag, default) pairs of integer arguments.  Without --shape: a fresh process per
    shape of `shapes`, each under `step_seconds`, nothing more started after a failure, their JSON lines collected into one.  With it
    (internal): run_shape(name, reps, *option values) in this process."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=reps)
    for flag, default in options:
        ap.add_argument(flag, type=int, default=default)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", default=None, help="(internal) run one shape in this process")
    args = ap.parse_args()
    values = [getattr(args, flag.lstrip("-")) for flag, _ in options]
    if args.shape:
        return run_shape(args.shape, args.reps, *values)
    passed_on = ["--reps", str(args.reps)] + [s for (flag, _), v in zip(options, values) for s in (flag, str(v))]
    res = {}
    for name in shapes:
        r = subprocess.run([sys.executable, os.path.abspath(script), "--shape", name, *passed_on], stdout=subprocess.PIPE, text=True,
                           timeout=step_seconds)
        if r.returncode != 0:
            raise SystemExit(f"{os.path.basename(script)}: shape {name} ended with status {r.returncode}; stopping")
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    emit(bench, res, args.out)
