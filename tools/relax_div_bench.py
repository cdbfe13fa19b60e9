"""What the divergence-form smoother and loss term cost (poisson.relax(form="divergence"), relax_kernel<DivOp> of
csrc/relax.hip; functional.physics_mse_loss(form="divergence"), physics_loss_kernel<DivLoss> of csrc/physics.hip).

    python tools/relax_div_bench.py [--out profiles/relax_div_bench.json]

1. The smoother.  E = 10 fields of 640^2 and E = 1024 of 80^2, theta ~ U(0.5, 2), both face means, 8 and 16 sweeps
   (one and two launches).  Three variants in one process, taking turns:
     (a) kernel     poisson.relax(form="divergence")
     (b) composed   the same sweeps from poisson.apply_div plus torch elementwise operations: the only route without
                    the kernel (one launch for D u and three elementwise ones per sweep; the node constants g and w
                    are formed once outside the timing, in its favour)
     (c) pointwise  poisson.relax at the same shape (another equation: the cost of the kernel it is modelled on)
   ms per call (``calls`` back to back between two HIP events, median of ``--reps`` alternating repeats) beside the
   traffic floor of a launch -- u, f, theta read and u written once, 32 bytes per node, at the 8.0 TB/s HBM peak of
   the MI355X -- and the fraction floor / measured.
2. The loss step.  B = 1024, n = 40, kinds alternating: forward + backward of physics_mse_loss with
   form="divergence" (both means), of the pointwise loss and of the plain MSE.

A recorded observation, not a pass criterion.  Needs a GPU: there is no fallback."""
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

HBM_PEAK = 8.0e12          # bytes / s, the MI355X's specified HBM3E peak
BYTES_PER_NODE = 32        # a launch reads u, f, theta and writes u, fp64
SHAPES = ((10, 640), (1024, 80))
MEANS = ("arithmetic", "harmonic")


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def composed(u, g, w, theta, mean, inv_h2, sweeps):
    """``sweeps`` Jacobi sweeps from apply_div: u + w (D u / inv_h2 - g), not the kernel's rounding order."""
    for _ in range(sweeps):
        u = torch.addcmul(u, w, P.apply_div(u, theta, mean, inv_h2).div_(inv_h2).sub_(g))
    return u


def smoother(reps, omega, calls):
    K = H.pde_relax_sweeps_per_launch()
    rows = []
    for E, n in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(n)
        u = torch.randn(E, n, n, generator=g, dtype=torch.float64, device="cuda") * 1e-4
        f = torch.randn(E, n, n, generator=g, dtype=torch.float64, device="cuda")
        theta = 0.5 + 1.5 * torch.rand(E, n, n, generator=g, dtype=torch.float64, device="cuda")
        inv_h2 = float((n - 1) ** 2)
        one = torch.ones_like(u)
        consts = {}
        yy, xx = torch.meshgrid(torch.arange(n, device="cuda"), torch.arange(n, device="cuda"), indexing="ij")
        red = ((yy + xx) % 2 == 0).to(torch.float64).expand(E, n, n).contiguous()
        for mean in MEANS:
            # the node constants of (b), outside the timing.  The sum of a node's four faces from apply_div alone:
            # on a red node D red = -(its four faces) inv_h2 (itself 1, its neighbours and the ghost ring 0)
            dr = -P.apply_div(red, theta, mean, inv_h2) / inv_h2
            db = -P.apply_div(one - red, theta, mean, inv_h2) / inv_h2
            consts[mean] = (f / inv_h2, omega / torch.where(red > 0, dr, db))
        variants = [("kernel", m) for m in MEANS] + [("composed", m) for m in MEANS] + [("pointwise", None)]

        def run(kind, mean, sweeps):
            if kind == "kernel":
                return P.relax(u, f, theta, sweeps, omega, form="divergence", face_mean=mean)
            if kind == "composed":
                return composed(u, *consts[mean], theta, mean, inv_h2, sweeps)
            return P.relax(u, f, theta, sweeps, omega)
        floor_ms = E * n * n * BYTES_PER_NODE / HBM_PEAK * 1e3
        for sweeps in (K, 2 * K):
            for kind, mean in variants:
                run(kind, mean, sweeps)
            for mean in MEANS:       # (b) is the same iteration as (a), to rounding
                a, b = run("kernel", mean, sweeps), run("composed", mean, sweeps)
                assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max()), (mean, sweeps)
            times = {v: [] for v in variants}
            for _ in range(reps):
                for v in variants:
                    times[v].append(timed_ms(lambda: [run(*v, sweeps) for _ in range(calls)]) / calls)
            launches = -(-sweeps // K)
            for v in variants:
                med = statistics.median(times[v])
                row = {"E": E, "n": n, "sweeps": sweeps, "variant": v[0], "face_mean": v[1], "ms": med,
                       "ms_min": min(times[v]), "ms_max": max(times[v])}
                if v[0] != "composed":
                    row.update(launches=launches, traffic_floor_ms_per_launch=floor_ms,
                               floor_over_measured=launches * floor_ms / med)
                rows.append(row)
                print(json.dumps(row), flush=True)
    return {"sweeps_per_launch": K, "tile": H.RELAX_TILE, "omega": omega, "hbm_peak_bytes_per_s": HBM_PEAK,
            "bytes_per_node_per_launch": BYTES_PER_NODE,
            "timing": "calls through poisson.relax / apply_div (output and workspace allocation from the caching "
                      "allocator included), %d back to back between two HIP events, median of alternating repeats"
                      % calls, "rows": rows}


def loss_step(reps, calls, B=1024, n=40):
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(B, 1, n, n, generator=g, device="cuda")
    y0 = t + 0.01 * torch.randn(B, 1, n, n, generator=g, device="cuda")
    x = torch.randn(B, 3, n, n, generator=g, device="cuda")
    x[:, 1] = (0.5 + 1.5 * torch.rand(B, n, n, generator=g, device="cuda") - 1.25) / 0.43
    kind = (torch.arange(B, device="cuda") % 2).to(torch.int32)
    stats = torch.tensor([0.3, 0.02, -0.1, 0.5, 1.25, 0.43], device="cuda")
    variants = {"divergence_arithmetic": lambda y: F.physics_mse_loss(y, t, x, kind, stats, 0.01, form="divergence",
                                                                       face_mean="arithmetic"),
                "divergence_harmonic": lambda y: F.physics_mse_loss(y, t, x, kind, stats, 0.01, form="divergence"),
                "pointwise": lambda y: F.physics_mse_loss(y, t, x, kind, stats, 0.01),
                "mse": lambda y: F.mse_loss(y, t)}

    def step(fn):
        y = y0.detach().requires_grad_(True)
        fn(y).backward()
    for fn in variants.values():
        step(fn)
    times = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            times[k].append(timed_ms(lambda: [step(fn) for _ in range(calls)]) / calls)
    rows = [{"variant": k, "ms": statistics.median(v), "ms_min": min(v), "ms_max": max(v)} for k, v in times.items()]
    for r in rows:
        print(json.dumps(r), flush=True)
    return {"B": B, "n": n, "timing": "loss forward + backward through autograd, %d back to back between two HIP "
                                      "events, median of alternating repeats" % calls, "rows": rows}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--omega", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relax_div_bench.json"))
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("relax_div_bench: no GPU (a timing needs one)")
    result = {"tool": "tools/relax_div_bench.py", "device": torch.cuda.get_device_name(0), "reps": a.reps,
              "smoother": smoother(a.reps, a.omega, a.calls), "loss_step": loss_step(a.reps, a.calls)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(result, indent=1) + "\n")
    return result


if __name__ == "__main__":
    main()
