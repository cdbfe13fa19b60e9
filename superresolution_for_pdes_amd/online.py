"""Training on an endless stream of freshly solved samples, generated on the device.

``SampleStream.next_batch()`` draws, solves and assembles one batch in the current stream: the wave numbers,
crop starts and (optionally) the coefficient field come from a counter-based generator on the GPU
(csrc/datastream.hip: Philox4x32-10, a pure function of (seed, global sample index, field, element)), the forcing
and the Poisson solves are the kernels the fixed dataset uses, one window pass crops / strides / casts the solved
fields and ``srpde_pde_dataset_assemble`` normalises them with FROZEN statistics.  Per batch there is no host draw,
no host->device copy of per-sample data (seed, indices and sizes are kernel arguments) and no host sync.  No sample
is seen twice.  The fixed, seeded dataset (train_enhanced.generate_on_device + PDEDataset) is untouched: this is a
second data source for the same ``train_model``.

Samples.  A batch of B has ``B - round(B * sub_fraction)`` standard samples in its first slots and subdomain
samples in the rest, so every shape is static.
  * standard  (reference data_generation.py): k1, k2 ~ U(k_std); independent solves on the fine and the coarse
    grid, f_coarse the forcing on the coarse grid, theta_coarse = theta_fine[::2, ::2];
  * subdomain (reference enhanced_data_generation.py): k1, k2 ~ U(k_sub); one solve on the super-fine grid, a
    random n_fine window (start_x, start_y in [0, n_superfine - n_fine)) and its stride-2 subsample.
theta is 1 (``theta_range=None``, what both reference generators train on) or U(theta_range) per pixel of the
solve grid (``(0.5, 2.0)`` is the distribution of the cascade and subdomain studies).

Operator.  ``form="pointwise"`` (default) solves theta * Lap(u) = f, as the reference does.  ``form="divergence"``
solves the conservative div(theta grad u) = f with ``face_mean`` on the cell faces instead -- every field (standard
fine / coarse, the super-fine subdomain solves, the calibration set) by poisson.solve_div with a fixed ``pcg_iters``
iterations, so a batch still needs no host sync.  It needs a ``theta_range``: with theta = 1 the two forms coincide.
Draws, crop starts, statistics arithmetic and sample identity are the same for both.

Sides.  ``bc`` (poisson.check_bc, e.g. ``"ddnn"``), with ``form="divergence"``: the three solves take zero-flux sides
(solve_div(bc=), the same fixed iteration count; the separable plans are built in the constructor).  ``"nnnn"`` is
singular without a shift and refused; ``"dddd"`` is no pattern.  ``describe()`` always carries ``bc``.
``state_dict()`` carries it only for a stream that has a pattern -- a stream without one keeps the two-key state it
always had, so earlier checkpoints still load -- and ``load_state_dict`` refuses a state whose pattern (or lack of
one) differs from the stream's: resuming under other sides would silently change the samples.

Boundary data.  ``boundary=(g_amp, q_amp)``, with ``form="divergence"``: every sample's walls carry smooth random data
from the generator's field 2 (srpde_stream_walls: four cosine modes per side) -- values g of amplitude ``g_amp`` beyond
the "d" sides of ``bc`` (all four sides without a pattern), outward fluxes q of amplitude ``q_amp`` through its "n"
sides -- and every solve (standard fine, standard coarse with the stride-2 data ``bd[..., ::2]``, as for theta; the
super-fine subdomain solves; calibration; validation) is ``solve_div(..., bc_data=)`` in the same fixed-iteration
mode: no host read, capturable.  A standard sample's [4, n_fine] fp32 data, in raw units, travels with the batch
(``next_batch(with_bd=True)``, ``fixed_set``'s "bd", ``FrozenSet.batch(idx, with_bd=True)``) for
``physics_mse_loss(bc_data=)``; a subdomain sample's row is zero and never read, its window's ring being unknown to
the loss anyway.  ``describe()`` always carries ``boundary``, ``state_dict()`` only when it is set, and
``load_state_dict`` refuses a mismatch, as for ``bc``.  None (default): nothing changes, bit for bit.

Global sample indices.  Local slot i of step t on rank r of ``world`` is sample
    s = (t * world + r) * B + i,
so a world of W ranks at step t consumes exactly the samples of the single-process steps t*W .. t*W + W - 1.  The
63-bit index space is split into three ranges that can never overlap:
    training     [0, 2^61)            next_batch (refuses to run past the end)
    calibration  [2^61, 2^62)         the frozen statistics: fixed_set(n_calib, CALIB_FIRST)
    validation   [2^62, 2^63)         held-out evaluation:   fixed_set(n, VALID_FIRST)
``fixed_set`` takes indices from the two held-out ranges only.

Frozen statistics.  ``stream.stats`` = (u_mean, u_std, f_mean, f_std, theta_mean, theta_std) in fp32, computed once
in the constructor from the calibration set with PDEDataset's arithmetic (fp32 mean, unbiased std, theta passed
through as (0, 1) when its std < 1e-6), then held fixed for every batch and for the validation set.
"""
from __future__ import annotations

import numpy as np
import torch

from . import hipops as H
from . import poisson as P

TRAIN_END = 1 << 61
CALIB_FIRST = 1 << 61
CALIB_END = 1 << 62
VALID_FIRST = 1 << 62
VALID_END = 1 << 63
HELD_OUT = ((CALIB_FIRST, CALIB_END), (VALID_FIRST, VALID_END))


def sample_indices(step: int, batch_size: int, rank: int = 0, world: int = 1) -> range:
    """The global sample indices of ``rank``'s batch at ``step``."""
    first = (step * world + rank) * batch_size
    return range(first, first + batch_size)


def n_standard(n: int, sub_fraction: float) -> int:
    """Standard samples among n slots (they come first); the other ``round(n * sub_fraction)`` are subdomain samples."""
    return n - int(round(n * sub_fraction))


def default_pcg_iters(theta_range, tol: float = 1e-12, margin: int = 4) -> int:
    """The fixed iteration count of form="divergence": the smallest k with 2 ((sqrt(c) - 1) / (sqrt(c) + 1))^k <= tol
    for c = theta_hi / theta_lo (CG's bound at the condition number that theta_max / theta_min bounds for the
    sine-preconditioned operator), plus ``margin``.  30 for (0.5, 2)."""
    lo, hi = (float(v) for v in theta_range)
    if not 0.0 < lo <= hi:
        raise ValueError(f"theta_range {theta_range}: 0 < lo <= hi")
    return P.pcg_iterations(lo, hi, tol) + margin     # the bound itself: also diffuse's, for any time step


def slot_kinds(n: int, sub_fraction: float) -> list:
    """The kind of each of n slots: 0 for the standard samples (first), 1 for the subdomain samples."""
    n_std = n_standard(n, sub_fraction)
    return [0] * n_std + [1] * (n - n_std)


class FrozenSet:
    """A fixed set normalised with a stream's frozen statistics: what DeviceBatchLoader needs of a PDEDataset.
    ``kind`` (optional): [N] int32 on the device, 0 = standard sample, 1 = subdomain sample.  ``bd`` (optional):
    [N, 4, n] fp32 on the device, the samples' boundary data in raw units (zero rows for subdomain samples)."""

    def __init__(self, inputs, targets, stats, kind=None, bd=None):
        self.inputs, self.targets, self.stats, self.kind, self.bd = inputs, targets, stats, kind, bd
        self.u_mean, self.u_std = stats[0], stats[1]

    def __len__(self):
        return self.inputs.shape[0]

    def __getitem__(self, idx):
        return self.inputs[idx], self.targets[idx]

    def batch(self, idx, with_kind: bool = False, with_bd: bool = False):
        if with_kind and self.kind is None:
            raise ValueError("FrozenSet: sample kinds were asked for, but the set was built without them")
        if with_bd and self.bd is None:
            raise ValueError("FrozenSet: boundary data was asked for, but the set was built without it")
        out = (self.inputs.index_select(0, idx), self.targets.index_select(0, idx))
        if with_kind:
            out += (self.kind.index_select(0, idx),)
        if with_bd:
            out += (self.bd.index_select(0, idx),)
        return out

    def denormalize(self, x):
        return x * self.u_std + self.u_mean


class SampleStream:
    def __init__(self, seed, batch_size, sub_fraction=0.5, k_std=(0.5, 5.0), k_sub=(0.5, 12.0), theta_range=None,
                 solver="dst", rank=0, world=1, device="cuda", n_coarse=20, n_fine=40, n_superfine=80, n_calib=2048,
                 form="pointwise", face_mean="harmonic", pcg_iters=None, bc=None, boundary=None):
        # (checked first: these refusals need no device)
        self.form = P.check_form(form)
        P.check_face_mean(face_mean)
        self.bc = None if P.check_bc(bc) is None else bc     # the pattern; "dddd" is no pattern
        if self.bc is not None and self.form != "divergence":
            raise ValueError('SampleStream: bc belongs to form="divergence" (the pointwise solvers have the zero '
                             "ghost ring)")
        if self.bc == "nnnn":
            raise ValueError('SampleStream: bc="nnnn" is singular without a shift (the constants): no unique sample')
        self.boundary = None
        if boundary is not None:
            if self.form != "divergence":
                raise ValueError('SampleStream: boundary belongs to form="divergence" (the pointwise solvers have the '
                                 "zero ghost ring)")
            try:
                g_amp, q_amp = (float(v) for v in boundary)
            except (TypeError, ValueError):
                raise ValueError(f"SampleStream: boundary = (g_amp, q_amp), got {boundary!r}") from None
            if not (np.isfinite(g_amp) and np.isfinite(q_amp)):
                raise ValueError(f"SampleStream: boundary = (g_amp, q_amp) must be finite, got {boundary!r}")
            self.boundary = (g_amp, q_amp)
        self._mask = P.check_bc(self.bc) or 0
        if self.form == "divergence":
            if theta_range is None:
                raise ValueError('SampleStream: form="divergence" needs a theta_range -- with theta = 1 it is the '
                                 "pointwise operator")
            self.face_mean = face_mean
            self.pcg_iters = default_pcg_iters(theta_range) if pcg_iters is None else int(pcg_iters)
            if self.pcg_iters < 1:
                raise ValueError("SampleStream: pcg_iters >= 1")
        else:
            if face_mean != "harmonic" or pcg_iters is not None:
                raise ValueError('SampleStream: face_mean and pcg_iters belong to form="divergence"')
            self.face_mean = self.pcg_iters = None
        if not str(device).startswith("cuda"):
            raise RuntimeError("SampleStream generates on a ROCm device (the HIP path has no CPU fallback)")
        if batch_size < 1 or not 0.0 <= sub_fraction <= 1.0:
            raise ValueError("batch_size >= 1 and 0 <= sub_fraction <= 1")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world {world}")
        if n_fine != 2 * n_coarse or n_superfine <= n_fine:
            raise ValueError("n_fine = 2 n_coarse (the stride-2 coarse grid) and n_superfine > n_fine (a window to draw)")
        self.seed, self.batch_size, self.sub_fraction = int(seed), int(batch_size), float(sub_fraction)
        self.k_std, self.k_sub = tuple(k_std), tuple(k_sub)
        self.theta_range = None if theta_range is None else tuple(float(v) for v in theta_range)
        self.solver = P.check_solver(solver)
        self.rank, self.world, self.device = int(rank), int(world), device
        self.n_coarse, self.n_fine, self.n_superfine = n_coarse, n_fine, n_superfine
        self.step = 0
        self.last_fields = None
        if self.solver == "dst" or self.form == "divergence":   # the plans are built here, never inside a step (or a stream capture)
            for n in (n_coarse, n_fine, n_superfine):
                P.dst_plan(n, device)
                if self.bc is not None:
                    P.sep_plan(n, self.bc, device)
        # frozen statistics, PDEDataset's arithmetic on the calibration set (the one host read of the stream)
        cal = self.fixed_set(n_calib, CALIB_FIRST)
        u_mean, u_std = cal["u_fine"].mean(), cal["u_fine"].std()
        f_mean, f_std = cal["f_fine"].mean(), cal["f_fine"].std()
        self.theta_is_constant = bool(cal["theta_fine"].std() < 1e-6)
        if self.theta_is_constant:
            t_mean, t_std = torch.zeros((), device=device), torch.ones((), device=device)
        else:
            t_mean, t_std = cal["theta_fine"].mean(), cal["theta_fine"].std()
        self.stats = torch.stack([u_mean, u_std, f_mean, f_std, t_mean, t_std]).float().contiguous()
        self.kind = self._kinds(self.batch_size)   # every batch has the same slots

    def _kinds(self, n: int):
        return torch.tensor(slot_kinds(n, self.sub_fraction), dtype=torch.int32, device=self.device)

    # ---- generation -------------------------------------------------------------------------------------------
    def _solve(self, f, theta, bd=None):
        if bd is not None:              # the same fixed mode, started from the data: four "d" sides without a pattern
            return P.solve_div(f, theta, face_mean=self.face_mean, bc=self.bc, precond_shift=0.0, maxit=self.pcg_iters,
                               check_every=0, check=False, device=self.device, bc_data=bd)
        if self.bc is not None:         # the same fixed mode with the separable preconditioner of those sides
            return P.solve_div(f, theta, face_mean=self.face_mean, bc=self.bc, precond_shift=0.0, maxit=self.pcg_iters,
                               check_every=0, check=False, device=self.device)
        if self.form == "divergence":   # fixed mode: pcg_iters iterations, no host sync, nothing read back
            return P.solve_div(f, theta, face_mean=self.face_mean, maxit=self.pcg_iters, check_every=0, check=False,
                               device=self.device)
        return P.solve_batched(f, theta, device=self.device, method=self.solver)

    def describe(self) -> dict:
        """What the stream generates: the settings a run records about its data source."""
        return {"seed": self.seed, "batch_size": self.batch_size, "sub_fraction": self.sub_fraction,
                "k_std": list(self.k_std), "k_sub": list(self.k_sub),
                "theta_range": None if self.theta_range is None else list(self.theta_range), "solver": self.solver,
                "form": self.form, "face_mean": self.face_mean, "pcg_iters": self.pcg_iters, "bc": self.bc,
                "boundary": None if self.boundary is None else list(self.boundary),
                "rank": self.rank, "world": self.world,
                "n_coarse": self.n_coarse, "n_fine": self.n_fine, "n_superfine": self.n_superfine}

    def _fields(self, first_index: int, n: int, keep: bool = False) -> dict:
        """The fp32 training fields of samples first_index .. first_index + n - 1 (standard slots first).
        ``keep``: also the fp64 fields behind them, under "fp64".  A stream with ``boundary``: also "bd" [n, 4, nf] fp32,
        the standard samples' boundary data and zero rows for the subdomain samples."""
        nc, nf, nsf, dev = self.n_coarse, self.n_fine, self.n_superfine, self.device
        n_std = n_standard(n, self.sub_fraction)
        n_sub = n - n_std
        f32 = dict(dtype=torch.float32, device=dev)
        out = {"u_fine": torch.empty(n, nf, nf, **f32), "f_fine": torch.empty(n, nf, nf, **f32),
               "theta_fine": torch.empty(n, nf, nf, **f32), "u_coarse": torch.empty(n, nc, nc, **f32)}
        order = ("u_fine", "f_fine", "theta_fine", "u_coarse")
        behind = {}
        walls = self.boundary is not None
        if walls:
            out["bd"] = torch.empty(n, 4, nf, **f32)
            if n_sub:
                out["bd"][n_std:].zero_()
        if n_std:
            k, _, th_f, th_c = H.stream_draw(self.seed, first_index, n_std, self.k_std, self.theta_range, n=nf,
                                             theta_half=True, device=dev)
            f_f, f_c = P.forcing_batched(k, nf, dev), P.forcing_batched(k, nc, dev)
            bd_f = bd_c = None
            if walls:
                bd_f, bd_c, _ = H.stream_walls(self.seed, first_index, n_std, nf, self._mask, self.boundary, half=True,
                                               f32=out["bd"][:n_std], device=dev)
            u_f, u_c = self._solve(f_f, th_f, bd_f), self._solve(f_c, th_c, bd_c)
            H.stream_window(u_f, f_f, th_f, None, nf, u_coarse_in=u_c, out=tuple(out[key][:n_std] for key in order))
            behind["standard"] = {"k12": k, "u_fine": u_f, "f_fine": f_f, "theta_fine": th_f, "u_coarse": u_c,
                                  "f_coarse": f_c, "theta_coarse": th_c}
            if walls:
                behind["standard"].update(bd=bd_f, bd_half=bd_c)
        if n_sub:
            k, starts, th, _ = H.stream_draw(self.seed, first_index + n_std, n_sub, self.k_sub, self.theta_range, n=nsf,
                                             max_start=nsf - nf, device=dev)
            f = P.forcing_batched(k, nsf, dev)
            bd = H.stream_walls(self.seed, first_index + n_std, n_sub, nsf, self._mask, self.boundary,
                                device=dev)[0] if walls else None
            u = self._solve(f, th, bd)
            H.stream_window(u, f, th, starts, nf, out=tuple(out[key][n_std:] for key in order))
            behind["subdomain"] = {"k12": k, "starts": starts, "u": u, "f": f, "theta": th}
            if walls:
                behind["subdomain"]["bd"] = bd
        flag = np.zeros(n, dtype=bool)
        flag[n_std:] = True
        out["is_subdomain"] = flag
        if keep:
            out["fp64"] = behind
        return out

    def _assemble(self, fields: dict):
        return H.pde_dataset_assemble(fields["u_coarse"], fields["u_fine"], fields["theta_fine"], fields["f_fine"],
                                      self.stats, self.theta_is_constant)

    def indices(self, step: int = None) -> range:
        """The global sample indices of this rank's batch at ``step`` (default: the next one)."""
        return sample_indices(self.step if step is None else step, self.batch_size, self.rank, self.world)

    def next_batch(self, keep_fields: bool = False, with_kind: bool = False, with_bd: bool = False):
        """(inputs [B, 3, nf, nf], targets [B, 1, nf, nf]) fp32, normalised with the frozen statistics; stream-ordered,
        no host sync.  ``keep_fields``: ``self.last_fields`` keeps the batch's fields, the fp64 solves included.
        ``with_kind``: a third element, the slots' kinds [B] int32 (0 standard, 1 subdomain; the same tensor every
        batch).  ``with_bd`` (a stream with ``boundary``): one more element after it, the batch's boundary data
        [B, 4, nf] fp32 in raw units, zero rows in the subdomain slots."""
        if with_bd and self.boundary is None:
            raise ValueError("SampleStream: with_bd needs a stream built with boundary=(g_amp, q_amp)")
        idx = self.indices()
        if idx.stop > TRAIN_END:
            raise RuntimeError("SampleStream: the training index range [0, 2^61) is used up")
        fields = self._fields(idx.start, self.batch_size, keep=keep_fields)
        self.last_fields = fields if keep_fields else None
        self.step += 1
        if with_kind or with_bd:
            return (*self._assemble(fields), *((self.kind,) if with_kind else ()),
                    *((fields["bd"],) if with_bd else ()))
        return self._assemble(fields)

    def fixed_set(self, n: int, first_index: int) -> dict:
        """The training fields (u_coarse, u_fine, f_fine, theta_fine in fp32 on the device, and the host flag
        is_subdomain -- what PDEDataset takes; with ``boundary`` also bd [n, 4, n_fine] fp32) of the n samples
        first_index .. first_index + n - 1 of a held-out range (CALIB_FIRST.. for calibration, VALID_FIRST.. for
        validation; module docstring)."""
        if n < 1 or not any(lo <= first_index and first_index + n <= hi for lo, hi in HELD_OUT):
            raise ValueError(f"fixed_set: samples [{first_index}, {first_index + n}) are not inside one held-out range "
                             f"(calibration [2^61, 2^62), validation [2^62, 2^63))")
        return self._fields(int(first_index), int(n))

    def frozen_set(self, n: int, first_index: int = VALID_FIRST) -> FrozenSet:
        """``fixed_set`` normalised with the frozen statistics (a validation set)."""
        fields = self.fixed_set(n, first_index)
        return FrozenSet(*self._assemble(fields), self.stats, self._kinds(n), fields.get("bd"))

    def validation_loader(self, n: int, batch_size: int = None, first_index: int = VALID_FIRST,
                          with_kind: bool = False, with_bd: bool = False):
        """A fixed validation loader over ``frozen_set(n, first_index)``: the single-process batches dealt to the
        ranks (DeviceBatchLoader's shard_batches), so the reduced loss equals the single-process one."""
        from .train_enhanced import DeviceBatchLoader
        return DeviceBatchLoader(self.frozen_set(n, first_index), batch_size or self.batch_size, shuffle=False,
                                 rank=self.rank, world=self.world, shard_batches=True, with_kind=with_kind,
                                 with_bd=with_bd)

    def denormalize(self, x):
        return x * self.stats[1] + self.stats[0]

    # ---- resuming ---------------------------------------------------------------------------------------------
    def state_dict(self) -> dict:
        state = {"seed": self.seed, "step": self.step}
        if self.bc is not None:             # a stream without a pattern keeps the state it always had
            state["bc"] = self.bc
        if self.boundary is not None:       # likewise
            state["boundary"] = list(self.boundary)
        return state

    def load_state_dict(self, state: dict):
        if state.get("bc") != self.bc:
            raise ValueError(f"SampleStream: the state belongs to bc={state.get('bc')!r}, this stream has {self.bc!r}")
        theirs = state.get("boundary")
        theirs = None if theirs is None else tuple(float(v) for v in theirs)
        if theirs != self.boundary:
            raise ValueError(f"SampleStream: the state belongs to boundary={theirs!r}, this stream has "
                             f"{self.boundary!r}")
        if int(state["seed"]) != self.seed:
            raise ValueError(f"SampleStream: the state belongs to seed {state['seed']}, this stream has {self.seed}")
        self.step = int(state["step"])


class OnlineBatchLoader:
    """``steps_per_epoch`` new batches of a SampleStream per pass: a train_loader for train_model."""

    def __init__(self, stream: SampleStream, steps_per_epoch: int, with_kind: bool = False, with_bd: bool = False):
        if steps_per_epoch < 1:
            raise ValueError("steps_per_epoch >= 1")
        if with_bd and stream.boundary is None:
            raise ValueError("OnlineBatchLoader: with_bd needs a stream built with boundary=(g_amp, q_amp)")
        if with_bd and not with_kind:       # train_model reads a batch by position: (inputs, targets, kind, bd)
            raise ValueError("OnlineBatchLoader: with_bd goes with with_kind=True (batches are read by position)")
        self.stream, self.steps_per_epoch, self.with_kind, self.with_bd = stream, int(steps_per_epoch), with_kind, with_bd

    def __len__(self):
        return self.steps_per_epoch

    def __iter__(self):
        for _ in range(self.steps_per_epoch):
            if self.with_bd:
                yield self.stream.next_batch(with_kind=self.with_kind, with_bd=True)
            else:
                yield self.stream.next_batch(with_kind=self.with_kind)

    def denormalize(self, x):
        return self.stream.denormalize(x)
