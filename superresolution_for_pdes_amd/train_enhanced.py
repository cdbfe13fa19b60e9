"""Drop-in for reference ``src/train_enhanced.py`` on MI355X.

``train_model`` keeps the reference signature and history dict (train_enhanced.py:15-139):
per batch zero_grad -> forward -> criterion -> backward -> clip_grad_norm_(grad_clip) ->
optimizer.step(); validation under no_grad; ReduceLROnPlateau on the val loss; best
checkpoint on improvement; early stopping.  Differences that do not change results:

* the batch loss is accumulated ON DEVICE and read once per epoch (the reference's
  per-batch ``loss.item()`` host sync, :77, is gone);
* with ``FusedAdamW`` the clip + update is one fused HIP pass (same math);
* batches are gathered by index on the device (``DeviceBatchLoader``) -- the reference's
  DataLoader workers (:286-300) cannot touch device tensors anyway;
* ``main`` accepts overrides (``--epochs``, ``--batch-size``, ``--data``, ``--generate``
  for on-device data generation, config #3, ``--online`` for a stream of new samples
  generated on the device, online.py) and runs data-parallel over RCCL when
  launched with torchrun (one process per GPU, distributed.DataParallel): the generated
  dataset's solves are sharded over the ranks and all-gathered, the batch size is per rank
  (global batch = world x batch), and validation deals the single-process batches to the
  ranks so the reduced val loss (which drives the scheduler, checkpoints and early stopping)
  equals the single-process value.
"""
from __future__ import annotations

import argparse
import json
import os
from datetime import datetime
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
import torch.nn as nn
import torch.optim as optim

from .functional import MSELoss
from .models import PDEDataset, UNet, init_weights
from .optim import FusedAdamW


class ScalarWriter:
    """TensorBoard-compatible add_scalar/close; uses torch.utils.tensorboard when installed,
    else appends JSON lines (same tags: 'Loss/train', 'Loss/val', 'Learning_rate')."""

    def __init__(self, log_dir):
        self.tb = None
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.tb = SummaryWriter(log_dir=log_dir)
        except Exception:  # tensorboard is optional (absent in this image)
            Path(log_dir).mkdir(parents=True, exist_ok=True)
            self.f = open(Path(log_dir) / "scalars.jsonl", "a")

    def add_scalar(self, tag, value, step):
        if self.tb is not None:
            self.tb.add_scalar(tag, value, step)
        else:
            self.f.write(json.dumps({"tag": tag, "value": float(value), "step": int(step)}) + "\n")
            self.f.flush()

    def close(self):
        if self.tb is not None:
            self.tb.close()
        else:
            self.f.close()


class DeviceBatchLoader:
    """Index-gathered batches from a device-resident PDEDataset (DataLoader replacement).

    shuffle: a seeded permutation per epoch; with world > 1 each rank takes a disjoint
    strided shard of it (DistributedSampler semantics: ``batch_size`` is per rank, the global
    batch is world x batch_size, as under torch DDP).  ``shard_batches`` (evaluation): the
    single-process batches themselves are dealt round-robin to the ranks, unpadded, so the
    all-reduced (sum of batch losses, batch count) gives exactly the single-process mean.
    ``with_kind``: batches are (inputs, targets, kind), the dataset's ``batch(idx, with_kind=True)``.
    ``with_bd``: one more element, the samples' boundary data (online.FrozenSet.batch(idx, with_kind, with_bd=True))."""

    def __init__(self, dataset, batch_size, shuffle=False, seed=0, rank=0, world=1, drop_last=False,
                 shard_batches=False, with_kind=False, with_bd=False):
        self.ds, self.bs, self.shuffle = dataset, batch_size, shuffle
        self.seed, self.rank, self.world, self.drop_last = seed, rank, world, drop_last
        self.shard_batches = shard_batches
        if with_bd and not with_kind:       # train_model reads a batch by position: (inputs, targets, kind, bd)
            raise ValueError("DeviceBatchLoader: with_bd goes with with_kind=True (batches are read by position)")
        self.with_kind = with_kind
        self.with_bd = with_bd
        self.epoch = 0

    def _indices(self):
        from .distributed import shard_indices
        n = len(self.ds)
        if self.world > 1 and not self.shard_batches:
            return shard_indices(n, self.rank, self.world, self.seed, self.epoch, self.shuffle)
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            return torch.randperm(n, generator=g)
        return torch.arange(n)

    def _batches(self, idx):
        out = [idx[s:s + self.bs] for s in range(0, len(idx), self.bs)]
        if self.drop_last and out and len(out[-1]) < self.bs:
            out = out[:-1]
        if self.shard_batches and self.world > 1:
            out = out[self.rank::self.world]
        return out

    def __len__(self):
        return len(self._batches(self._indices()))

    def __iter__(self):
        idx = self._indices().to(self.ds.inputs.device)
        self.epoch += 1
        for b in self._batches(idx):
            if self.with_bd:
                yield self.ds.batch(b, with_kind=self.with_kind, with_bd=True)
                continue
            yield self.ds.batch(b, with_kind=True) if self.with_kind else self.ds.batch(b)


def _is_main():
    return not dist.is_initialized() or dist.get_rank() == 0


def _global_mean(total, count, device):
    """(sum of batch losses, number of batches) summed over ranks -> the mean batch loss, the
    reference's ``loss_sum / len(loader)`` (train_enhanced.py:79, :92) over all ranks' batches."""
    t = torch.stack([total.to(torch.float64), torch.tensor(float(count), dtype=torch.float64, device=device)])
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t)
    return float(t[0] / torch.clamp(t[1], min=1.0))


def _global_means(totals, count, device):
    """``_global_mean`` for a vector of sums sharing one batch count -> a list of means (one all-reduce)."""
    t = torch.cat([totals.to(torch.float64), torch.tensor([float(count)], dtype=torch.float64, device=device)])
    if dist.is_initialized() and dist.get_world_size() > 1:
        dist.all_reduce(t)
    return (t[:-1] / torch.clamp(t[-1], min=1.0)).tolist()


def _unpack(batch, device):
    """(inputs, targets, kind or None, bd or None) of a 2-, 3- or 4-tuple batch (inputs, targets[, kind[, bd]]), on
    ``device``.  Read by position: boundary data is always the fourth element, which is why the loaders refuse
    ``with_bd`` without ``with_kind``."""
    inputs, targets = batch[0].to(device), batch[1].to(device)
    return (inputs, targets, (batch[2].to(device) if len(batch) > 2 else None),
            (batch[3].to(device) if len(batch) > 3 else None))


def _criterion_call(criterion, outputs, targets, inputs, kind, bd=None):
    if getattr(criterion, "needs_inputs", False):
        if kind is None:
            raise ValueError("this criterion needs (inputs, targets, kind) batches: build the loaders with "
                             "with_kind=True")
        if getattr(criterion, "needs_bd", False):
            if bd is None:
                raise ValueError("this criterion needs (inputs, targets, kind, bd) batches: build the loaders with "
                                 "with_kind=True, with_bd=True")
            return criterion(outputs, targets, inputs, kind, bd)
        return criterion(outputs, targets, inputs, kind)
    return criterion(outputs, targets)


def train_model(model: nn.Module, train_loader, val_loader, criterion: nn.Module, optimizer: optim.Optimizer,
                scheduler, num_epochs: int, device: str, save_dir: Path, writer, grad_clip: float = 1.0,
                early_stopping_patience: int = 20) -> dict:
    """Train with per-epoch validation, checkpointing and early stopping (train_enhanced.py:15-139)."""
    history = {"train_loss": [], "val_loss": [], "best_val_loss": float("inf"), "best_epoch": 0, "num_epochs": 0}
    no_improvement_count = 0
    save_dir = Path(save_dir)
    fused = isinstance(optimizer, FusedAdamW)
    module = model.module if hasattr(model, "module") else model
    # a criterion with ``needs_inputs`` (functional.PhysicsMSELoss) is called with the batch's inputs and kinds and
    # reports its (total, mse, pde) terms: four more history lists, accumulated and reduced like the loss
    terms = getattr(criterion, "needs_inputs", False)
    if terms:
        history.update({"train_mse": [], "train_pde": [], "val_mse": [], "val_pde": []})
    for epoch in range(num_epochs):
        model.train()
        acc = torch.zeros((), dtype=torch.float64, device=device)
        tacc = torch.zeros(2, dtype=torch.float64, device=device) if terms else None
        nb = 0
        for batch in train_loader:
            inputs, targets, kind, bd = _unpack(batch, device)
            optimizer.zero_grad()
            outputs = model(inputs)
            loss = _criterion_call(criterion, outputs, targets, inputs, kind, bd)
            loss.backward()
            if fused:
                optimizer.step(max_grad_norm=grad_clip)
            else:
                torch.nn.utils.clip_grad_norm_(module.parameters(), grad_clip)
                optimizer.step()
            acc += loss.detach()
            if terms:
                tacc += criterion.last_terms[1:]
            nb += 1
        train_loss = _global_mean(acc, nb, device)
        if terms:
            train_mse, train_pde = _global_means(tacc, nb, device)

        # under data parallelism each rank's last training forward updated its BN running
        # statistics with its own shard: validate every rank with rank 0's buffers (the state
        # best_model.pth saves), so the reduced val loss is that model's single-process loss
        if hasattr(model, "sync_buffers"):
            model.sync_buffers()
        model.eval()
        vacc = torch.zeros((), dtype=torch.float64, device=device)
        vtacc = torch.zeros(2, dtype=torch.float64, device=device) if terms else None
        vb = 0
        with torch.no_grad():
            for batch in val_loader:
                inputs, targets, kind, bd = _unpack(batch, device)
                vacc += _criterion_call(criterion, model(inputs), targets, inputs, kind, bd).detach()
                if terms:
                    vtacc += criterion.last_terms[1:]
                vb += 1
        val_loss = _global_mean(vacc, vb, device)
        if terms:
            val_mse, val_pde = _global_means(vtacc, vb, device)
            for key, v in (("train_mse", train_mse), ("train_pde", train_pde), ("val_mse", val_mse),
                           ("val_pde", val_pde)):
                history[key].append(v)

        scheduler.step(val_loss)
        current_lr = optimizer.param_groups[0]["lr"]
        if writer is not None:
            writer.add_scalar("Loss/train", train_loss, epoch)
            writer.add_scalar("Loss/val", val_loss, epoch)
            writer.add_scalar("Learning_rate", current_lr, epoch)
        history["train_loss"].append(train_loss)
        history["val_loss"].append(val_loss)
        if _is_main():
            print(f"Epoch {epoch + 1}/{num_epochs}:\nTrain Loss: {train_loss:.6f}\nVal Loss: {val_loss:.6f}\n"
                  f"Learning Rate: {current_lr:.6f}")
        if val_loss < history["best_val_loss"]:
            history["best_val_loss"] = val_loss
            history["best_epoch"] = epoch
            no_improvement_count = 0
            if _is_main():
                torch.save({"epoch": epoch, "model_state_dict": module.state_dict(),
                            "optimizer_state_dict": optimizer.state_dict(),
                            "scheduler_state_dict": scheduler.state_dict(),
                            "train_loss": train_loss, "val_loss": val_loss}, save_dir / "best_model.pth")
                print(f"Saved new best model with val_loss: {val_loss:.6f}")
        else:
            no_improvement_count += 1
            if _is_main():
                print(f"No improvement for {no_improvement_count} epochs (best: {history['best_val_loss']:.6f} "
                      f"at epoch {history['best_epoch'] + 1})")
        if no_improvement_count >= early_stopping_patience:
            if _is_main():
                print(f"Early stopping triggered after {epoch + 1} epochs")
            break
    history["num_epochs"] = len(history["train_loss"])
    return history


def plot_losses(history: dict, save_dir: Path):
    """training_history.png (train_enhanced.py:141-183)."""
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except Exception:
        return
    plt.figure(figsize=(12, 7))
    epochs = range(1, len(history["train_loss"]) + 1)
    plt.plot(epochs, history["train_loss"], "b-", label="Training Loss")
    plt.plot(epochs, history["val_loss"], "r-", label="Validation Loss")
    be = history["best_epoch"] + 1
    plt.plot(be, history["best_val_loss"], "go", markersize=10,
             label=f"Best Model (Epoch {be}, Loss: {history['best_val_loss']:.6f})")
    plt.xlabel("Epoch")
    plt.ylabel("Loss")
    plt.title("Training and Validation Loss")
    plt.legend()
    plt.grid(True, alpha=0.3)
    plt.tight_layout()
    plt.savefig(Path(save_dir) / "training_history.png", dpi=150)
    plt.close()


def stratified_split(data, val_split=0.2, stratify=True):
    """Index split with the reference's np.random call order (train_enhanced.py:232-268)."""
    n_samples = len(data["u_fine"])
    indices = np.random.permutation(n_samples)
    val_size = int(n_samples * val_split)
    if stratify and "is_subdomain" in data:
        sub = np.where(data["is_subdomain"])[0]
        std = np.where(~data["is_subdomain"])[0]
        np.random.shuffle(sub)
        np.random.shuffle(std)
        vs, vt = int(len(sub) * val_split), int(len(std) * val_split)
        train_idx = np.concatenate([std[vt:], sub[vs:]])
        val_idx = np.concatenate([std[:vt], sub[:vs]])
        np.random.shuffle(train_idx)
        np.random.shuffle(val_idx)
    else:
        train_idx, val_idx = indices[val_size:], indices[:val_size]
    return train_idx, val_idx


def default_config():
    """The reference's config dict (train_enhanced.py:192-205)."""
    return {
        "batch_size": 32, "num_epochs": 500, "learning_rate": 2e-4, "min_lr": 1e-6, "patience": 10,
        "early_stopping_patience": 20, "val_split": 0.2, "grad_clip": 1.0,
        "device": "cuda" if torch.cuda.is_available() else "cpu",
        "num_workers": 4, "pin_memory": True, "stratify_by_subdomain": True,
    }


def generate_on_device(n_standard=1000, n_subdomain=1000, keep_on_device=True, shard=None, solver="cg"):
    """Config #3: the enhanced_data_generation.py __main__ dataset built by the HIP solver.
    The fields stay device tensors from the batched CG to PDEDataset; under
    torchrun the solves are sharded over the ranks and all-gathered (8(e)), the draws global.
    ``solver``: "cg" or "dst" (poisson.solve_batched's method)."""
    from .enhanced_data_generation import EnhancedPoissonSolver
    s = EnhancedPoissonSolver(20, 40, 80, solver=solver)
    d1 = s.generate_dataset(n_samples=n_standard, k_range=(0.5, 5.0), keep_on_device=keep_on_device, shard=shard)
    d2 = s.generate_subdomain_dataset(n_samples=n_subdomain, k_range=(0.5, 12.0), keep_on_device=keep_on_device,
                                      shard=shard)
    return s.combine_datasets(d1, d2)


def _per_sample(v):
    return (v.ndim if hasattr(v, "ndim") else np.ndim(v)) > 0


def select(data: dict, idx) -> dict:
    """Rows ``idx`` of every per-sample field (device tensors indexed on the device)."""
    out = {}
    for k, v in data.items():
        if not _per_sample(v):
            continue
        out[k] = v[torch.as_tensor(idx, device=v.device)] if isinstance(v, torch.Tensor) else v[idx]
    return out


def arg_parser():
    ap = argparse.ArgumentParser(description="MI355X U-Net training (reference train_enhanced.main)")
    ap.add_argument("--data", default="data/pde_dataset.npz")
    ap.add_argument("--generate", type=int, nargs=2, metavar=("N_STD", "N_SUB"), default=None,
                    help="generate the dataset on device instead of loading --data")
    ap.add_argument("--epochs", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None,
                    help="per-rank batch (under torchrun the global batch is world x batch-size, as torch DDP)")
    ap.add_argument("--results", default="results")
    ap.add_argument("--solver", choices=("cg", "dst"), default="cg",
                    help="Poisson solver of --generate / --online: conjugate gradients (default) or the direct sine "
                         "transform")
    ap.add_argument("--online", type=int, metavar="STEPS_PER_EPOCH", default=None,
                    help="train on a stream of new samples generated on the device (online.SampleStream), this many "
                         "batches per epoch, instead of a fixed dataset")
    ap.add_argument("--online-theta", type=float, nargs=2, metavar=("LO", "HI"), default=None,
                    help="with --online: theta ~ U(LO, HI) per pixel instead of theta = 1")
    ap.add_argument("--pde-weight", type=float, default=0.0, metavar="LAMBDA",
                    help="add LAMBDA x the mean squared residual of the discrete equation to the MSE loss "
                         "(functional.PhysicsMSELoss); 0 (default): plain MSE")
    ap.add_argument("--pde-div-weight", type=float, default=0.0, metavar="LAMBDA",
                    help="add LAMBDA x the mean squared residual of div(theta grad u) = f to the MSE loss "
                         "(functional.PhysicsMSELoss(form='divergence')); needs --operator divergence and uses its "
                         "--face-mean; not together with --pde-weight")
    ap.add_argument("--operator", choices=("pointwise", "divergence"), default="pointwise",
                    help="the equation behind the --online samples: theta * Lap(u) = f (default) or the conservative "
                         "div(theta grad u) = f (poisson.solve_div; needs --online and --online-theta)")
    ap.add_argument("--face-mean", choices=("arithmetic", "harmonic"), default="harmonic",
                    help="with --operator divergence: the mean of the two nodal theta on a cell face")
    ap.add_argument("--bc", default=None, metavar="PATTERN",
                    help='with --online and --operator divergence: the sides of the samples\' problem, four of "d" '
                         '(zero ghost ring) / "n" (zero flux) for (row 0, row n-1, column 0, column n-1), e.g. ddnn; '
                         "it reaches the stream, the validation set and the --pde-div-weight term")
    ap.add_argument("--bc-data", type=float, nargs=2, metavar=("G_AMP", "Q_AMP"), default=None,
                    help="with --online and --operator divergence: smooth random boundary data on every sample's walls "
                         "(online.SampleStream(boundary=)): values of amplitude G_AMP beyond the \"d\" sides of --bc "
                         "(all four without it), outward fluxes of amplitude Q_AMP through its \"n\" sides; it reaches "
                         "the stream, the validation set and the --pde-div-weight term")
    return ap


def check_operator_args(args):
    """The refusals of --operator / --face-mean / --pde-div-weight / --bc / --bc-data, before any device work."""
    if getattr(args, "bc_data", None) is not None:
        if args.online is None or args.operator != "divergence":
            raise SystemExit("--bc-data needs --online and --operator divergence (the pointwise solvers and the fixed "
                             "dataset generators have the zero ghost ring)")
        if not all(np.isfinite(v) for v in args.bc_data):
            raise SystemExit("--bc-data: two finite amplitudes G_AMP Q_AMP")
    if args.bc is not None:
        from .poisson import check_bc
        try:
            mask = check_bc(args.bc)
        except ValueError as e:
            raise SystemExit(f"--bc: {e}")
        if args.online is None or args.operator != "divergence":
            raise SystemExit("--bc needs --online and --operator divergence (the pointwise solvers and the fixed "
                             "dataset generators have the zero ghost ring)")
        if mask == 15:
            raise SystemExit("--bc nnnn is singular without a shift (the constants): no unique sample")
    if args.pde_div_weight < 0:
        raise SystemExit("--pde-div-weight: a weight >= 0")
    if args.pde_div_weight > 0:
        if args.operator != "divergence":
            raise SystemExit("--pde-div-weight weighs the residual of div(theta grad u) = f: it needs --operator "
                             "divergence (--pde-weight is the pointwise residual's weight)")
        if args.pde_weight > 0:
            raise SystemExit("--pde-div-weight cannot be combined with --pde-weight > 0: a run's samples solve one "
                             "equation")
    if args.operator == "divergence":
        if args.online is None or args.online_theta is None:
            raise SystemExit("--operator divergence needs --online and --online-theta (with theta = 1 it is the "
                             "pointwise operator, and the fixed dataset generators are pointwise)")
        if args.pde_weight > 0:
            raise SystemExit("--operator divergence cannot be combined with --pde-weight > 0: that flag weighs the "
                             "pointwise residual theta * Lap(u) - f, which these samples do not satisfy; "
                             "--pde-div-weight weighs the residual of div(theta grad u) = f")
    elif args.face_mean != "harmonic":
        raise SystemExit("--face-mean belongs to --operator divergence")


ONLINE_VAL_SAMPLES = 400   # the fixed validation set of --online (the default dataset's split: 20 % of 2000)


def online_loaders(args, config, rank, world, device):
    """The loaders of --online: an endless training stream (seed 42, as the rest of main) and a fixed validation
    set from its held-out indices, both normalised with the stream's frozen statistics."""
    from .online import OnlineBatchLoader, SampleStream
    if args.online < 1:
        raise SystemExit("--online: at least one step per epoch")
    stream = SampleStream(42, config["batch_size"], theta_range=args.online_theta, solver=args.solver, rank=rank,
                          world=world, device=device, form=args.operator, face_mean=args.face_mean, bc=args.bc,
                          boundary=None if args.bc_data is None else tuple(args.bc_data))
    with_kind = args.pde_weight > 0 or args.pde_div_weight > 0
    if args.bc_data is not None and args.pde_div_weight > 0:   # the term needs the walls the samples were solved with
        return (OnlineBatchLoader(stream, args.online, with_kind=True, with_bd=True),
                stream.validation_loader(ONLINE_VAL_SAMPLES, config["batch_size"], with_kind=True, with_bd=True))
    return (OnlineBatchLoader(stream, args.online, with_kind=with_kind),
            stream.validation_loader(ONLINE_VAL_SAMPLES, config["batch_size"], with_kind=with_kind))


def physics_criterion(weight, stats, save_dir=None, form="pointwise", face_mean="harmonic", bc=None, bc_data=None):
    """The criterion of --pde-weight (``form="pointwise"``) or --pde-div-weight (``"divergence"``, with the run's
    ``face_mean`` and ``bc``; ``bc_data``: the run's --bc-data amplitudes, and the criterion then takes each batch's
    boundary data); with ``save_dir`` its settings go to physics_loss.json beside config.json."""
    from .functional import PhysicsMSELoss
    criterion = PhysicsMSELoss(weight, stats, form=form, face_mean=face_mean, bc=bc, bc_data=bc_data is not None)
    if save_dir is not None:
        with open(Path(save_dir) / "physics_loss.json", "w") as f:
            json.dump({"weight": criterion.weight, "inv_h2": list(criterion.inv_h2),
                       "stats": [float(v) for v in stats.detach().cpu()], "form": criterion.form,
                       "face_mean": criterion.face_mean if form == "divergence" else None, "bc": criterion.bc,
                       "bc_data": None if bc_data is None else [float(v) for v in bc_data]},
                      f, indent=4)
    return criterion


def main(argv=None):
    args = arg_parser().parse_args(argv)
    if args.online_theta is not None and args.online is None:
        raise SystemExit("--online-theta needs --online")
    if args.pde_weight < 0:
        raise SystemExit("--pde-weight: a weight >= 0")
    check_operator_args(args)
    with_kind = args.pde_weight > 0 or args.pde_div_weight > 0

    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1 and not dist.is_initialized():
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    rank = dist.get_rank() if dist.is_initialized() else 0

    torch.manual_seed(42)
    np.random.seed(42)
    torch.cuda.manual_seed(42)
    config = default_config()
    if args.epochs is not None:
        config["num_epochs"] = args.epochs
    if args.batch_size is not None:
        config["batch_size"] = args.batch_size
    device = f"cuda:{torch.cuda.current_device()}" if torch.cuda.is_available() else "cpu"

    save_dir = Path(args.results) / f"enhanced_run_{datetime.now().strftime('%Y%m%d_%H%M%S')}"
    if rank == 0:
        save_dir.mkdir(parents=True, exist_ok=True)
        recorded = dict(config)
        if args.operator != "pointwise":   # (the pointwise run's config.json keeps the reference's keys)
            recorded.update(operator=args.operator, face_mean=args.face_mean)
        if args.bc is not None:
            recorded.update(bc=args.bc)
        if args.bc_data is not None:
            recorded.update(bc_data=list(args.bc_data))
        with open(save_dir / "config.json", "w") as f:
            json.dump(recorded, f, indent=4)
    writer = ScalarWriter(str(save_dir / "tensorboard")) if rank == 0 else None

    if args.online is not None:
        train_loader, val_loader = online_loaders(args, config, rank, world, device)
        stats = train_loader.stream.stats
    else:
        if args.generate is not None:
            data = generate_on_device(*args.generate, solver=args.solver)
        else:
            data = dict(np.load(args.data))
        train_idx, val_idx = stratified_split(data, config["val_split"], config["stratify_by_subdomain"])
        train_ds = PDEDataset(select(data, train_idx), device=device)
        val_ds = PDEDataset(select(data, val_idx), device=device)
        train_loader = DeviceBatchLoader(train_ds, config["batch_size"], shuffle=True, seed=42, rank=rank, world=world,
                                         with_kind=with_kind)
        val_loader = DeviceBatchLoader(val_ds, config["batch_size"], shuffle=False, rank=rank, world=world,
                                       shard_batches=True, with_kind=with_kind)
        stats = train_ds.stats

    model = UNet().to(device)
    model.apply(init_weights)
    net = model
    if world > 1:
        from .distributed import DataParallel
        net = DataParallel(model)
    if args.pde_div_weight > 0:
        criterion = physics_criterion(args.pde_div_weight, stats, save_dir if rank == 0 else None, "divergence",
                                      args.face_mean, args.bc, args.bc_data)
    elif with_kind:
        criterion = physics_criterion(args.pde_weight, stats, save_dir if rank == 0 else None)
    else:
        criterion = MSELoss()
    optimizer = FusedAdamW(model.parameters(), lr=config["learning_rate"], weight_decay=1e-4)
    scheduler = optim.lr_scheduler.ReduceLROnPlateau(optimizer, mode="min", factor=0.5, patience=config["patience"],
                                                     min_lr=config["min_lr"])
    history = train_model(net, train_loader, val_loader, criterion, optimizer, scheduler, config["num_epochs"],
                          device, save_dir, writer, config["grad_clip"], config["early_stopping_patience"])
    if rank == 0:
        plot_losses(history, save_dir)
        torch.save({"epoch": len(history["train_loss"]) - 1, "model_state_dict": model.state_dict(),
                    "optimizer_state_dict": optimizer.state_dict(), "scheduler_state_dict": scheduler.state_dict(),
                    "train_loss": history["train_loss"][-1], "val_loss": history["val_loss"][-1],
                    "best_val_loss": history["best_val_loss"], "best_epoch": history["best_epoch"]},
                   save_dir / "final_model.pth")
        print(f"\nTraining Summary:\nTotal epochs: {len(history['train_loss'])}\n"
              f"Best validation loss: {history['best_val_loss']:.6f} (epoch {history['best_epoch'] + 1})")
        writer.close()
    return history


if __name__ == "__main__":
    main()
