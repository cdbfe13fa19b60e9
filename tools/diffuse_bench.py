"""Time implicit time stepping of u_t = div(theta grad u) - f (poisson.diffuse: the shifted sine-preconditioned CG,
warm-started from the previous state) and the shifted solve beside the stationary one.

    python tools/diffuse_bench.py [--out profiles/diffuse_bench.json] [--repeats 7]

Per (n, B) and dt: theta ~ U(0.5, 2) per pixel, f the project's forcing with k ~ U(0.5, 12) (rng 100), u(0) = 0,
backward Euler, the harmonic mean (diffuse's default), rtol 1e-12.
(i)   ``--steps`` steps in tolerance mode: poisson.diffuse (every solve starts from the previous state) against the
      same steps with every solve started from zero (rhs by torch arithmetic, poisson.solve_div(shift=)): ms per step
      and the iterations of each step (the batch's maximum).
(ii)  ``--graph-steps`` steps in fixed mode (pcg_iters = the largest warm count of (i) plus 2, precond_shift given):
      eager, and the same loop captured once in a graph and replayed.  The graph's result is checked to be the eager
      one's bits.
(iii) One shifted solve from zero, solve_div(shift=1/dt), against solve_div at shift 0 on the same f and theta: ms
      and iterations.
All variants of one (n, B, dt) take turns inside each repeat; HIP-event time per call, the median of the repeats with
min - max, after a warm-up call.  There is no variant that composes the step from the pre-shift interface: apply_div
plus torch arithmetic can form the right-hand side, but solve_div without a shift cannot solve (D_theta - sigma I) u =
rhs at all, so there is nothing to time.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from superresolution_for_pdes_amd import poisson as P  # noqa: E402

SIZES = "80:1024,640:4"
DTS = "1e-2,1e-4,1e-6"
LO, HI = 0.5, 2.0


def timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def summary(ms, per=1):
    return {"ms": round(statistics.median(ms) / per, 4), "ms_min": round(min(ms) / per, 4),
            "ms_max": round(max(ms) / per, 4)}


def alternating(fns, repeats):
    """{name: [ms per call]}: one warm-up call each, then the variants taking turns inside every repeat."""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn))
    return ms


def zero_started(f, th, sigma, sigma_p, steps):
    """The same backward-Euler steps with every solve started from zero -> (u, [steps, B] iterations)."""
    u = torch.zeros_like(f)
    counts = []
    for _ in range(steps):
        u, it, _ = P.solve_div(f - sigma * u, th, return_info=True, shift=sigma, precond_shift=sigma_p)
        counts.append(it)
    return u, torch.stack(counts)


def bench(n, B, dt, rng, args):
    f = P.forcing_batched(rng.uniform(0.5, 12.0, (B, 2)), n)
    th = torch.from_numpy(rng.uniform(LO, HI, (B, n, n))).cuda()
    u0 = torch.zeros_like(f)
    P.dst_plan(n)
    sigma = 1.0 / dt
    sigma_p = P.precond_shift_for(th, sigma)
    row = {"n": n, "B": B, "dt": dt, "sigma": sigma, "sigma_p": sigma_p, "steps": args.steps,
           "graph_steps": args.graph_steps}

    u_w, warm = P.diffuse(u0, th, f, dt=dt, steps=args.steps, precond_shift=sigma_p, check=True)
    u_z, zero = zero_started(f, th, sigma, sigma_p, args.steps)
    row["warm_iters_per_step"] = warm.max(dim=1).values.tolist()
    row["zero_iters_per_step"] = zero.max(dim=1).values.tolist()
    row["warm_vs_zero_rel_diff"] = float((u_w - u_z).norm() / u_z.norm())
    k = int(warm.max()) + 2
    row["pcg_iters"] = k
    _, it0, _ = P.solve_div(f, th, return_info=True)
    _, its, _ = P.solve_div(f, th, return_info=True, shift=sigma, precond_shift=sigma_p)
    row["solve_iters"] = {"shift_0": int(it0.max()), "shifted": int(its.max())}

    kw = dict(dt=dt, steps=args.graph_steps, pcg_iters=k, precond_shift=sigma_p)
    eager = P.diffuse(u0, th, f, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = P.diffuse(u0, th, f, **kw)
    g.replay()
    torch.cuda.synchronize()
    row["graph_equals_eager"] = bool(torch.equal(out, eager))

    ms = alternating({
        "warm": lambda: P.diffuse(u0, th, f, dt=dt, steps=args.steps, precond_shift=sigma_p),
        "zero": lambda: zero_started(f, th, sigma, sigma_p, args.steps),
        "fixed_eager": lambda: P.diffuse(u0, th, f, **kw),
        "fixed_graph": g.replay,
        "solve_shift_0": lambda: P.solve_div(f, th),
        "solve_shifted": lambda: P.solve_div(f, th, shift=sigma, precond_shift=sigma_p),
    }, args.repeats)
    row["warm_ms_per_step"] = summary(ms["warm"], args.steps)
    row["zero_ms_per_step"] = summary(ms["zero"], args.steps)
    row["fixed_eager_ms_per_step"] = summary(ms["fixed_eager"], args.graph_steps)
    row["fixed_graph_ms_per_step"] = summary(ms["fixed_graph"], args.graph_steps)
    row["solve_shift_0"] = summary(ms["solve_shift_0"])
    row["solve_shifted"] = summary(ms["solve_shifted"])
    del g, out
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="n:B pairs")
    ap.add_argument("--dts", default=DTS)
    ap.add_argument("--steps", type=int, default=20, help="steps of the tolerance-mode loops of (i)")
    ap.add_argument("--graph-steps", type=int, default=100, help="steps of the fixed-mode loops of (ii)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("diffuse_bench: no GPU")
    rng = np.random.default_rng(100)
    rows = []
    for n, B in [tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",") if s]:
        for dt in [float(v) for v in args.dts.split(",") if v]:
            rows.append(bench(n, B, dt, rng, args))
            print(json.dumps(rows[-1]), flush=True)
    rec = {"tool": "tools/diffuse_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around one call (a whole loop of steps, or one solve); median of alternating repeats "
                     "after one warm-up call; the whole process, no kernel traced alone",
           "setup": f"theta ~ U({LO}, {HI}) per pixel, backward Euler, harmonic mean, rtol 1e-12, u(0) = 0",
           "bound": {"pcg_iterations": P.pcg_iterations(LO, HI)},
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return rec


if __name__ == "__main__":
    main()
