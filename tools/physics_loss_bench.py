"""Time the MSE + PDE-residual loss (functional.PhysicsMSELoss, csrc/physics.hip) on one GPU and record what the
term does to a short training run.

    python tools/physics_loss_bench.py [--out profiles/physics_loss_bench.json] [--batch 1024] [--repeats 7]

(i)   The loss alone at the training shape [B, 1, 40, 40]: physics forward (with the unit gradient) + backward against
      srpde_mse_fwd + srpde_mse_bwd, alternating, (a) as eager calls (host launch work included) and (b) replayed from
      a captured graph (the device time of the launches alone).  From (b) and the bytes each variant has to move, the
      fraction of the HBM peak.
(ii)  The training step of train_model (zero_grad, forward, loss, backward, fused clip + AdamW) with PhysicsMSELoss
      against the same step with MSELoss, same process, alternating; the difference of the medians beside the
      run-to-run spread (max - min) of the repeats.
(iii) ``--online-steps`` training steps on the sample stream at each weight of ``--weights``, seeded alike, then the
      validation set's (mse, pde) under no_grad: a recorded observation, not a pass criterion.
Needs a GPU: there is no fallback."""
import argparse
import itertools
import json
import os
import statistics
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from superresolution_for_pdes_amd import hipops as H  # noqa: E402
from superresolution_for_pdes_amd import online as O  # noqa: E402
from superresolution_for_pdes_amd.functional import DEFAULT_INV_H2, MSELoss, PhysicsMSELoss  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def timed_ms(fn, calls=1):
    """HIP-event milliseconds per call of ``calls`` back-to-back calls."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(calls):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / calls


def summary(ms):
    return {"ms": round(statistics.median(ms), 5), "ms_min": round(min(ms), 5), "ms_max": round(max(ms), 5)}


def alternating(fns, repeats, calls):
    """{name: [ms per call] * repeats}, the variants taking turns inside every repeat."""
    ms = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            ms[k].append(timed_ms(fn, calls))
    return ms


def captured(fn):
    """``fn`` as a graph replay (after a warm-up on a side stream)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def bench_loss(args):
    B, n = args.batch, 40
    g = torch.Generator(device="cuda").manual_seed(0)
    t = torch.randn(B, 1, n, n, device="cuda", generator=g)
    y = t + 0.05 * torch.randn(B, 1, n, n, device="cuda", generator=g)
    x = torch.randn(B, 3, n, n, device="cuda", generator=g)
    kind = torch.tensor(O.slot_kinds(B, 0.5), dtype=torch.int32, device="cuda")
    stats = torch.tensor([0.0, 0.01, 0.0, 0.5, 0.0, 1.0], device="cuda")
    gout = torch.ones((), device="cuda")

    def physics():
        _, unit = H.physics_loss_fwd(y, t, x, kind, stats, 0.01, DEFAULT_INV_H2)
        H.physics_loss_bwd(unit, gout)

    def mse():
        H.mse_fwd(y, t)
        H.mse_bwd(y, t, gout)
    plane = B * n * n * 4
    # y, t read + dy written (twice over for mse: fwd and bwd each read y and t); physics adds theta, f and the unit
    # gradient's write and read
    nbytes = {"mse": 5 * plane, "physics": 7 * plane}
    rows = {}
    for mode, wrap in (("eager", lambda f: f), ("graph", captured)):
        fns = {"mse": wrap(mse), "physics": wrap(physics)}
        for fn in fns.values():
            fn()
        torch.cuda.synchronize()
        ms = alternating(fns, args.repeats, args.loss_calls)
        rows[mode] = {k: summary(v) for k, v in ms.items()}
        rows[mode]["physics_minus_mse_ms"] = round(rows[mode]["physics"]["ms"] - rows[mode]["mse"]["ms"], 5)
    for k in ("mse", "physics"):
        gbs = nbytes[k] / (rows["graph"][k]["ms"] * 1e-3) / 1e9
        rows["graph"][k].update({"bytes": nbytes[k], "gb_per_s": round(gbs, 1),
                                 "hbm_fraction": round(gbs / HBM_PEAK_GBS, 4)})
    rec = {"batch": B, "n": n, "calls_per_window": args.loss_calls, "launches": {"mse": 3, "physics": 3}, **rows}
    print(json.dumps(rec), flush=True)
    return rec


def bench_step(args):
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.optim import FusedAdamW
    from superresolution_for_pdes_amd.train_enhanced import DeviceBatchLoader
    torch.manual_seed(42)
    stream = O.SampleStream(42, args.batch, solver="dst", n_calib=args.calib)
    fixed = DeviceBatchLoader(stream.frozen_set(2 * args.batch, O.CALIB_FIRST), args.batch, shuffle=True, seed=42,
                              with_kind=True)
    model = UNet().to("cuda")
    model.apply(init_weights)
    model.train()
    criteria = {"mse": MSELoss(), "physics": PhysicsMSELoss(0.01, stream.stats)}
    opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-4)
    acc = torch.zeros((), dtype=torch.float64, device="cuda")

    def feed():
        while True:
            yield from fixed
    src = feed()

    def step_with(name):
        crit = criteria[name]

        def step():
            inputs, targets, kind = next(src)
            opt.zero_grad()
            out = model(inputs)
            loss = crit(out, targets, inputs, kind) if name == "physics" else crit(out, targets)
            loss.backward()
            opt.step(max_grad_norm=1.0)
            acc.add_(loss.detach())
        return step
    fns = {k: step_with(k) for k in criteria}
    for fn in itertools.chain.from_iterable([fns.values()] * args.warmup):
        fn()
    torch.cuda.synchronize()
    ms = alternating(fns, args.repeats, args.steps)
    a, b = summary(ms["mse"]), summary(ms["physics"])
    spread = max(a["ms_max"] - a["ms_min"], b["ms_max"] - b["ms_min"])
    rec = {"batch": args.batch, "steps_per_window": args.steps, "step_mse": a, "step_physics": b,
           "physics_minus_mse_ms": round(b["ms"] - a["ms"], 4),
           "physics_minus_mse_percent": round(100.0 * (b["ms"] - a["ms"]) / a["ms"], 3),
           "run_to_run_spread_ms": round(spread, 4), "loss_finite": bool(torch.isfinite(acc))}
    print(json.dumps(rec), flush=True)
    return rec


def online_runs(args):
    from superresolution_for_pdes_amd.models import UNet, init_weights
    from superresolution_for_pdes_amd.optim import FusedAdamW
    from superresolution_for_pdes_amd.train_enhanced import train_model
    rows = []
    for weight in args.weights:
        torch.manual_seed(42)
        stream = O.SampleStream(42, args.online_batch, solver="dst")
        train = O.OnlineBatchLoader(stream, args.online_steps, with_kind=True)
        val = stream.validation_loader(400, args.online_batch, with_kind=True)
        model = UNet().to("cuda")
        model.apply(init_weights)
        opt = FusedAdamW(model.parameters(), lr=2e-4, weight_decay=1e-4)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=0.5, patience=10, min_lr=1e-6)
        crit = PhysicsMSELoss(weight, stream.stats) if weight > 0 else MSELoss()
        with tempfile.TemporaryDirectory() as tmp:
            hist = train_model(model, train, val, crit, opt, sched, 1, "cuda", tmp, None)
        probe = PhysicsMSELoss(max(weight, 0.01), stream.stats)     # the terms do not depend on the weight
        model.eval()
        tot = torch.zeros(2, dtype=torch.float64, device="cuda")
        nb = 0
        with torch.no_grad():
            for inputs, targets, kind in val:
                probe(model(inputs), targets, inputs, kind)
                tot += probe.last_terms[1:]
                nb += 1
        val_mse, val_pde = (tot / nb).tolist()
        row = {"weight": weight, "steps": args.online_steps, "batch": args.online_batch, "seed": 42,
               "train_loss": hist["train_loss"][-1], "val_loss": hist["val_loss"][-1], "val_mse": val_mse,
               "val_pde": val_pde}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--loss-calls", type=int, default=200, help="loss evaluations per timed window")
    ap.add_argument("--steps", type=int, default=10, help="training steps per timed window")
    ap.add_argument("--warmup", type=int, default=3, help="warm-up steps per criterion")
    ap.add_argument("--calib", type=int, default=2048, help="calibration samples of the frozen statistics")
    ap.add_argument("--online-steps", type=int, default=200)
    ap.add_argument("--online-batch", type=int, default=32)
    ap.add_argument("--weights", type=float, nargs="*", default=[0.0, 0.01])
    ap.add_argument("--out", default=None, help="also write the JSON record here")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("physics_loss_bench: no GPU")
    rec = {"tool": "tools/physics_loss_bench.py", "device": torch.cuda.get_device_name(0), "repeats": args.repeats,
           "timing": "HIP events around a window of back-to-back calls, per call; median of alternating repeats after "
                     "warm-up, with min and max",
           "loss_alone": bench_loss(args), "training_step": bench_step(args), "online_runs": online_runs(args)}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
    print(json.dumps(rec))
    return rec


if __name__ == "__main__":
    main()
