"""What a boundary pattern costs in the smoother, the loss step and the sample stream (ABI 23: poisson.relax(bc=),
functional.physics_mse_loss(bc=), online.SampleStream(bc=)), each against the same call without a pattern in the same
process.

    python tools/bc_path_bench.py [--out profiles/bc_path_bench.json]

1. The smoother.  E = 10 fields of 640^2 and E = 1024 of 80^2, theta ~ U(0.5, 2), harmonic faces, 8 and 16 sweeps (one
   and two launches): bc None, "ddnn", "nnnn".  The sweep loop is the same code; only the once-per-launch face
   formation differs.
2. The loss step.  B = 1024, n = 40, kinds alternating: forward + backward of physics_mse_loss(form="divergence") with
   bc None and "ddnn".
3. One streamed batch of 1024, SampleStream(form="divergence", theta_range=(0.5, 2)) with bc None and "ddnn": the three
   fixed-iteration solves with the sine-transform and with the separable preconditioner, the windows and the assembly.

ms per call (``calls`` back to back between two HIP events, median of ``--reps`` alternating repeats, every variant in
one process) and the ratio to the pattern-less variant of the same run.  Whole calls with the Python wrapper; no kernel
alone, no counters.  A recorded observation, not a pass criterion.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from superresolution_for_pdes_amd import functional as F  # noqa: E402
from superresolution_for_pdes_amd import hipops as H  # noqa: E402
from superresolution_for_pdes_amd import poisson as P  # noqa: E402
from superresolution_for_pdes_amd.online import SampleStream  # noqa: E402

SHAPES = ((10, 640), (1024, 80))


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(variants, reps, calls):
    """{name: fn} -> rows of medians over ``reps`` rounds in which the variants take turns, with the ratio to the
    first variant (the pattern-less one)."""
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed_ms(lambda: [fn() for _ in range(calls)]) / calls)
    base = statistics.median(times[next(iter(variants))])
    rows = []
    for k, v in times.items():
        med = statistics.median(v)
        rows.append({"bc": k, "ms": med, "ms_min": min(v), "ms_max": max(v), "ratio_to_none": med / base})
    return rows


def smoother(reps, omega, calls):
    K = H.pde_relax_sweeps_per_launch()
    rows = []
    for E, n in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n)
        u = torch.randn(E, n, n, generator=g, dtype=torch.float64, device="cuda") * 1e-4
        f = torch.randn(E, n, n, generator=g, dtype=torch.float64, device="cuda")
        theta = 0.5 + 1.5 * torch.rand(E, n, n, generator=g, dtype=torch.float64, device="cuda")
        for sweeps in (K, 2 * K):
            variants = {str(bc): (lambda bc=bc: P.relax(u, f, theta, sweeps, omega, form="divergence", bc=bc))
                        for bc in (None, "ddnn", "nnnn")}
            for row in alternate(variants, reps, calls):
                row = {"E": E, "n": n, "sweeps": sweeps, **row}
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"sweeps_per_launch": K, "omega": omega, "face_mean": "harmonic",
            "timing": "calls through poisson.relax (output and workspace allocation from the caching allocator "
                      "included), %d back to back between two HIP events, median of alternating repeats" % calls,
            "rows": rows}


def loss_step(reps, calls, B=1024, n=40):
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(B, 1, n, n, generator=g, device="cuda")
    y0 = t + 0.01 * torch.randn(B, 1, n, n, generator=g, device="cuda")
    x = torch.randn(B, 3, n, n, generator=g, device="cuda")
    x[:, 1] = (0.5 + 1.5 * torch.rand(B, n, n, generator=g, device="cuda") - 1.25) / 0.43
    kind = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], device="cuda")

    def step(bc):
        y = y0.detach().requires_grad_(True)
        F.physics_mse_loss(y, t, x, kind, stats, 0.01, form="divergence", bc=bc).backward()
    rows = alternate({str(bc): (lambda bc=bc: step(bc)) for bc in (None, "ddnn")}, reps, calls)
    for r in rows:
        print(json.dumps(r), flush=True)
    return {"B": B, "n": n, "face_mean": "harmonic",
            "timing": "loss forward + backward through autograd, %d back to back between two HIP events, median of "
                      "alternating repeats" % calls, "rows": rows}


def streamed_batch(reps, calls, B=1024):
    streams = {str(bc): SampleStream(42, B, theta_range=(0.5, 2.0), form="divergence", bc=bc, n_calib=256)
               for bc in (None, "ddnn")}
    rows = alternate({k: s.next_batch for k, s in streams.items()}, reps, calls)
    for r in rows:
        print(json.dumps(r), flush=True)
    s = streams["None"]
    return {"batch_size": B, "pcg_iters": s.pcg_iters, "sizes": [s.n_coarse, s.n_fine, s.n_superfine],
            "timing": "SampleStream.next_batch (draws, forcing, three fixed-iteration solves, windows, assembly), %d "
                      "back to back between two HIP events, median of alternating repeats" % calls, "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--stream-calls", type=int, default=2)
    ap.add_argument("--omega", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bc_path_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bc_path_bench: no GPU (a timing needs one)")
    result = {"tool": "tools/bc_path_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
              "smoother": smoother(a.reps, a.omega, a.calls), "loss_step": loss_step(a.reps, a.calls),
              "streamed_batch": streamed_batch(a.reps, a.stream_calls)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
