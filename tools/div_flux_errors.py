"""Measure, on the CPU, the tolerance that tests/test_gpu_div_flux.py holds ``poisson.effective_coefficient`` to.

    python tools/div_flux_errors.py [--out profiles/div_flux_errors.json]

The device solves by the preconditioned CG at rtol 1e-12; the closed forms and the dense adjoint gradient it is compared
with are exact.  What the iteration's stop rule leaves is measured here with the same iteration in numpy
(tests/div_bd_ref.py, pcg) against a dense solve on the test's own inputs (tests/div_flux_ref.py, effective_cases and the
gradient's random theta), relative to the value (for the gradient: to its largest entry).  The bound is 10 x the largest
figure: the device's reduction order differs from numpy's.  Needs no GPU."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import div_flux_ref as F  # noqa: E402
import poisson_div_ref as D  # noqa: E402

RTOL = 1e-12
SIZES = (6, 40)
GRAD_N, GRAD_B, GRAD_SEED = 6, 3, 11
MARGIN = 10.0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    values, grads = [], []
    for n in SIZES:
        for axis in (0, 1):
            theta, _ = F.effective_cases(n, axis)
            for mean in D.MEANS:
                for case, th in enumerate(theta):
                    dense = F.effective_coefficient(th, axis, mean)
                    pcg = F.effective_coefficient(th, axis, mean, solver="pcg", rtol=RTOL)
                    values.append({"n": n, "axis": axis, "mean": mean, "case": case,
                                   "rel_diff": abs(pcg - dense) / abs(dense)})
    theta = D.field_theta(GRAD_N, GRAD_SEED, 0.5, 2.0, GRAD_B)
    for axis in (0, 1):
        for mean in D.MEANS:
            for b, th in enumerate(theta):
                dense = F.effective_coefficient_grad(th, axis, mean)
                pcg = F.effective_coefficient_grad(th, axis, mean, solver="pcg", rtol=RTOL)
                grads.append({"n": GRAD_N, "axis": axis, "mean": mean, "problem": b,
                              "rel_diff": float(np.abs(pcg - dense).max() / np.abs(dense).max())})
    worst_v, worst_g = max(r["rel_diff"] for r in values), max(r["rel_diff"] for r in grads)
    rec = {"tool": "tools/div_flux_errors.py", "rtol": RTOL, "margin": MARGIN,
           "what": "numpy PCG (the device's iteration) against a dense solve, relative; bound = margin x the largest",
           "value": {"measured": worst_v, "bound": MARGIN * worst_v, "cases": values},
           "gradient": {"measured": worst_g, "bound": MARGIN * worst_g, "cases": grads}}
    print(json.dumps({"value": rec["value"]["measured"], "value_bound": rec["value"]["bound"],
                      "gradient": worst_g, "gradient_bound": rec["gradient"]["bound"]}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    return rec


if __name__ == "__main__":
    main()
