"""Time the face fluxes of the divergence-form operator, their wall totals and the effective coefficient beside the only
route there was without them: the same fields composed from torch slicing.

    python tools/div_flux_bench.py [--out profiles/div_flux_bench.json] [--repeats 7]

Per (n, B): theta ~ U(0.5, 2) per pixel, u ~ N(0, 1), the harmonic mean, for bc None (no data) and "ddnn" with random
data ~ N(0, 1) per problem.
    face_flux   poisson.face_flux              kernel | sliced: Fx, Fy from torch slicing | apply: poisson.apply_div
    wall_flux   poisson.wall_flux              kernel | sliced: four edge expressions and sums
    effective   poisson.effective_coefficient  full   | solve: its own solve_div alone (tolerance mode, rtol 1e-12)
``face_flux`` reads u and theta and writes two fields: 32 B per node.  ``floor_ms`` is that traffic at 8.0 TB/s and
``vs_floor`` the kernel's time over it; ``vs_apply`` its time over apply_div's of the same run (24 B per node).  Every
timing is of a whole Python call -- argument checks, output allocation and the launches -- so small shapes show the
wrapper, not the kernel.  All variants of one (n, B, bc) take turns inside each repeat; HIP-event time, the median of the
repeats with min - max, after a warm-up call.  Each (n, B, bc) step runs under its own time limit (``--step-timeout``
seconds of SIGALRM, which ends the process: nothing more is started on the GPU after a step that hangs).  Needs a GPU:
there is no fallback."""
import argparse
import json
import os
import signal
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from superresolution_for_pdes_amd import poisson as P  # noqa: E402

SIZES = "80:1024,640:4"
LO, HI = 0.5, 2.0
BCS = (None, "ddnn")
HBM_TBS = 8.0


def timed_ms(fn):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end)


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


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


def _side(bc, s):
    return bc is not None and bc[s] == "n"


def _walls(u, th, bd, bc, inv_h):
    """The outward flux through the wall faces of the four sides, [B, n] each, from torch slicing."""
    edges = ((slice(None), 0, slice(None)), (slice(None), -1, slice(None)), (slice(None), slice(None), 0),
             (slice(None), slice(None), -1))
    out = []
    for s, e in enumerate(edges):
        d = torch.zeros_like(u[e]) if bd is None else bd[:, s]
        out.append(d if _side(bc, s) else th[e] * (d - u[e]) * inv_h)
    return out


def sliced_face_flux(u, th, bd, bc):
    B, n = u.shape[0], u.shape[-1]
    inv_h = float(n - 1)
    Fx, Fy = u.new_empty(B, n, n + 1), u.new_empty(B, n + 1, n)
    ta, tb = th[:, :, :-1], th[:, :, 1:]
    Fx[:, :, 1:n] = 2.0 * ta * tb / (ta + tb) * (u[:, :, 1:] - u[:, :, :-1]) * inv_h
    ta, tb = th[:, :-1, :], th[:, 1:, :]
    Fy[:, 1:n, :] = 2.0 * ta * tb / (ta + tb) * (u[:, 1:, :] - u[:, :-1, :]) * inv_h
    w = _walls(u, th, bd, bc, inv_h)
    Fy[:, 0, :], Fy[:, n, :], Fx[:, :, 0], Fx[:, :, n] = -w[0], w[1], -w[2], w[3]
    return Fx, Fy


def sliced_wall_flux(u, th, bd, bc):
    n = u.shape[-1]
    return torch.stack([w.sum(-1) for w in _walls(u, th, bd, bc, float(n - 1))], dim=1) / float(n - 1)


def name(bc):
    return "dddd(None)" if bc is None else bc


def bench(n, B, bc, rng, args):
    th = torch.from_numpy(rng.uniform(LO, HI, (B, n, n))).cuda()
    u = torch.from_numpy(rng.standard_normal((B, n, n))).cuda()
    bd = None if bc is None else torch.from_numpy(rng.standard_normal((B, 4, n))).cuda()
    for axis in (0, 1):
        P.sep_plan(n, P.EFFECTIVE_PATTERNS[axis])
    zero = torch.zeros_like(th)
    unit = P.bc_data(n, "ddnn", row0=1.0)
    got, want = P.face_flux(u, th, bc=bc, bc_data=bd), sliced_face_flux(u, th, bd, bc)
    scale = max(float(want[0].abs().max()), float(want[1].abs().max()))
    agree = max(float((got[0] - want[0]).abs().max()), float((got[1] - want[1]).abs().max())) / scale
    fns = {
        ("face_flux", "kernel"): lambda: P.face_flux(u, th, bc=bc, bc_data=bd),
        ("face_flux", "sliced"): lambda: sliced_face_flux(u, th, bd, bc),
        ("face_flux", "apply"): lambda: P.apply_div(u, th, bc=bc, bc_data=bd),
        ("wall_flux", "kernel"): lambda: P.wall_flux(u, th, bc=bc, bc_data=bd),
        ("wall_flux", "sliced"): lambda: sliced_wall_flux(u, th, bd, bc),
    }
    if bc is not None:                 # the effective coefficient has its own sides: timed once per shape
        fns["effective", "full"] = lambda: P.effective_coefficient(th)
        fns["effective", "solve"] = lambda: P.solve_div(zero, th, bc="ddnn", bc_data=unit)
    out = {}
    for (kind, variant), t in alternating(fns, args.repeats).items():
        out.setdefault(kind, {})[variant] = summary(t)
    ff = out["face_flux"]
    floor_ms = 32.0 * B * n * n / (HBM_TBS * 1e12) * 1e3
    ff["floor_ms"] = round(floor_ms, 5)
    ff["vs_floor"] = round(ff["kernel"]["ms"] / floor_ms, 2)
    ff["vs_apply"] = round(ff["kernel"]["ms"] / ff["apply"]["ms"], 3)
    ff["sliced_over_kernel"] = round(ff["sliced"]["ms"] / ff["kernel"]["ms"], 2)
    ff["max_rel_diff_to_sliced"] = agree
    out["wall_flux"]["sliced_over_kernel"] = round(out["wall_flux"]["sliced"]["ms"] / out["wall_flux"]["kernel"]["ms"], 2)
    if "effective" in out:
        out["effective"]["full_over_solve"] = round(out["effective"]["full"]["ms"] / out["effective"]["solve"]["ms"], 3)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sizes", default=SIZES, help="n:B pairs")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one (n, B, bc) step may take")
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("div_flux_bench: no GPU")
    rng = np.random.default_rng(100)
    rows = []
    for n, B in [tuple(int(v) for v in s.split(":")) for s in args.sizes.split(",") if s]:
        row = {"n": n, "B": B, "bc": {}}
        for bc in BCS:
            signal.alarm(args.step_timeout)        # the default action ends the process
            row["bc"][name(bc)] = bench(n, B, bc, rng, args)
            signal.alarm(0)
        rows.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/div_flux_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around one whole Python call (checks, allocation, launches); median of alternating "
                     "repeats after one warm-up call; all variants in one process, no kernel traced alone",
           "setup": f"theta ~ U({LO}, {HI}) per pixel, u ~ N(0, 1), harmonic mean, data ~ N(0, 1) per problem for "
                    f"\"ddnn\"; floor = 32 B per node at {HBM_TBS} TB/s; effective = effective_coefficient(theta) "
                    "against its own solve_div (rtol 1e-12, tolerance mode)",
           "rows": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return rec


if __name__ == "__main__":
    main()
