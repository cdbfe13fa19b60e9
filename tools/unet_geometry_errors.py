"""Measure the errors that tests/test_gpu_unet_geometry.py holds to the project's bars, case by case.

    python tools/unet_geometry_errors.py [--out profiles/unet_geometry_errors.json] [--cpu]

The cases and the helper are the test's own (TRAIN_CASES / EVAL_CASES, step_figures, reference_conditioning).  Per
case one JSON line: the worst parameter gradient (relative L2 against the fp64 oracle on the HIP forward's branch)
with its name and the oracle's own fp32 error e32 on that branch, the output rmse over its std, the input-gradient
error; for the training cases also the reference's conditioning there (no GPU needed: the oracle's fp32 step on its
own branch against its fp64 step, worst parameter that is no conv bias feeding BN; a case needs <= 1e-1).
``--cpu``: only that conditioning figure (no GPU).  The bars stay the tests' (1e-4 / 3 e32 / 3e-5 / 5e-6 / 1e-5):
the record shows how far below them the paths sit."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_gpu_unet_geometry as G  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--cpu", action="store_true", help="only the reference's conditioning per training case (no GPU)")
    args = ap.parse_args(argv)
    records = []
    if not args.cpu:
        from superresolution_for_pdes_amd import hipops as H
    conditioning = {}
    for case in G.TRAIN_CASES:
        B, Hh, W, math = case
        rec = {"case": G.case_id(case), "mode": "train", "shape": [B, Hh, W], "conv_math": math}
        if (B, Hh, W) not in conditioning:
            name, e = G.reference_conditioning(B, Hh, W)
            conditioning[(B, Hh, W)] = {"worst_param": name, "fp32_vs_fp64_own_branch": e, "needs": 1e-1}
        rec["reference_conditioning"] = conditioning[(B, Hh, W)]
        if not args.cpu:
            before = H.conv_math()
            try:
                H.set_conv_math(math)
                rec.update(G.summary(G.step_figures(B, Hh, W, True)))
            finally:
                H.set_conv_math(before)
        records.append(rec)
        print(json.dumps(rec), flush=True)
    if not args.cpu:
        for case in G.EVAL_CASES:
            rec = {"case": G.case_id(case), "mode": "eval", "shape": list(case), "conv_math": "h3"}
            rec.update(G.summary(G.step_figures(*case, False)))
            records.append(rec)
            print(json.dumps(rec), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump({"tool": "tools/unet_geometry_errors.py",
                       "what": "HIP U-Net step against the fp64 oracle on the HIP forward's branch, relative L2; "
                               "e32: the oracle's own fp32 error on that branch",
                       "bars": {"param_and_dx_train": "max(1e-4, 3 e32)", "param_and_dx_eval": 1e-4,
                                "out_train": 3e-5, "out_eval": 5e-6, "zero_bias": 1e-4, "running": 1e-5},
                       "cases": records}, fh, indent=1)
            fh.write("\n")
    return records


if __name__ == "__main__":
    main()
