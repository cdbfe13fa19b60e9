"""What boundary data costs in the sample stream and the loss step (ABI 23 extended: online.SampleStream(boundary=),
functional.physics_mse_loss(bc_data=)), each against the same call without data in the same process.

    python tools/stream_bd_bench.py [--out profiles/stream_bd_bench.json]

1. One streamed batch of 1024 (grids 20 / 40 / 80), SampleStream(form="divergence", theta_range=(0.5, 2)) with bc None
   and "ddnn", each without and with boundary=(0.05, 0.1): with data a batch has two more launches (the wall synthesis
   of the standard and of the subdomain samples) and each of its three solves starts from srpde_div_cg_init_from_bd.
2. The loss step.  B = 1024, n = 40, kinds alternating: forward + backward of physics_mse_loss(form="divergence") with
   bc None and "ddnn", each without and with bc_data [B, 4, n].

ms per call (``calls`` back to back between two HIP events, median of ``--reps`` alternating repeats with their range,
every variant in one process) and the ratio to the data-less variant of the same pattern in the same run.  Whole calls
with the Python wrapper; no kernel alone, no counters.  A recorded observation, not a pass criterion.  Needs a GPU:
there is no fallback."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from superresolution_for_pdes_amd import functional as F  # noqa: E402
from superresolution_for_pdes_amd.online import SampleStream  # noqa: E402

PATTERNS = (None, "ddnn")
AMPS = (0.05, 0.1)


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(variants, reps, calls):
    """{(bc, data): fn} -> rows of medians over ``reps`` rounds in which the variants take turns, with the ratio to
    the data-less variant of the same pattern."""
    for fn in variants.values():
        fn()
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed_ms(lambda: [fn() for _ in range(calls)]) / calls)
    rows = []
    for (bc, data), v in times.items():
        med, base = statistics.median(v), statistics.median(times[bc, False])
        rows.append({"bc": str(bc), "data": data, "ms": med, "ms_min": min(v), "ms_max": max(v),
                     "ratio_to_no_data": med / base})
    return rows


def streamed_batch(reps, calls, B=1024):
    streams = {(bc, data): SampleStream(42, B, theta_range=(0.5, 2.0), form="divergence", bc=bc, n_calib=256,
                                        boundary=AMPS if data else None)
               for bc in PATTERNS for data in (False, True)}
    rows = alternate({k: ((lambda s=s: s.next_batch(with_bd=True)) if k[1] else s.next_batch)
                      for k, s in streams.items()}, reps, calls)
    for r in rows:
        print(json.dumps(r), flush=True)
    s = streams[None, False]
    return {"batch_size": B, "pcg_iters": s.pcg_iters, "sizes": [s.n_coarse, s.n_fine, s.n_superfine],
            "boundary": list(AMPS),
            "timing": "SampleStream.next_batch (draws, walls, forcing, three fixed-iteration solves, windows, assembly), "
                      "%d back to back between two HIP events, median of alternating repeats" % calls, "rows": rows}


def loss_step(reps, calls, B=1024, n=40):
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(B, 1, n, n, generator=g, device="cuda")
    y0 = t + 0.01 * torch.randn(B, 1, n, n, generator=g, device="cuda")
    x = torch.randn(B, 3, n, n, generator=g, device="cuda")
    x[:, 1] = (0.5 + 1.5 * torch.rand(B, n, n, generator=g, device="cuda") - 1.25) / 0.43
    kind = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], device="cuda")
    bd = 0.05 * torch.randn(B, 4, n, generator=g, device="cuda")

    def step(bc, data):
        y = y0.detach().requires_grad_(True)
        F.physics_mse_loss(y, t, x, kind, stats, 0.01, form="divergence", bc=bc,
                           **({"bc_data": bd} if data else {})).backward()
    rows = alternate({(bc, data): (lambda bc=bc, data=data: step(bc, data)) for bc in PATTERNS for data in (False, True)},
                     reps, calls)
    for r in rows:
        print(json.dumps(r), flush=True)
    return {"B": B, "n": n, "face_mean": "harmonic",
            "timing": "loss forward + backward through autograd, %d back to back between two HIP events, median of "
                      "alternating repeats" % calls, "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--stream-calls", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bd_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("stream_bd_bench: no GPU (a timing needs one)")
    result = {"tool": "tools/stream_bd_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
              "streamed_batch": streamed_batch(a.reps, a.stream_calls), "loss_step": loss_step(a.reps, a.calls)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
