"""Sweeps of the Gaussian experiment: the reference's YAML grids (Gaussian_experiment/configs/*.yaml, expanded as main.py:159-167
expands them) run in groups through the grouped fused step (``gaussian.fused.GroupedTrainer``): two launches per training step
and one evaluation forward for a whole group of runs, whatever their widths, batch sizes, modes and seeds.

Every run's log, parameters and optimizer state are bit for bit those of the same point run alone through ``build_run(fused=True)``
and ``train_model_steps_fused``.  The alignment metrics of an evaluation are one ``umlh.align.measure_pairs`` call for the whole group
(DESIGN section 27)."""
from __future__ import annotations

from itertools import product

import torch

from .data import generate_data
from .fused import FusedTrainer, GroupedTrainer
from .train import build_run

DEFAULT_GROUP_SIZE = 48     # the group size with the best member-step in profiles/gaussian_sweep_bench.txt

# main.py:174-192, the keys a grid may leave out
DEFAULTS = dict(dim_obs=50, dim_common=100, dim_latent=128, batch_size=512, num_steps=1000, lr=1e-3, data_dim_common=5, data_dim_x=10,
                data_dim_y=10, noise_std=0.1, train_num_samples=100000, val_num_samples=2000, seed=0, alpha_x=1.0, alpha_y=1.0, mode="xy",
                tag="default", attenuation=0.05, unrelated_info=False)

_DATA_KEYS = ("train_num_samples", "val_num_samples", "data_dim_common", "data_dim_x", "data_dim_y", "dim_obs", "noise_std", "attenuation")
_DATA = {}          # the values of _DATA_KEYS -> (train, train2, val) host dicts
_DEVICE_DATA = {}   # (device, the values of _DATA_KEYS) -> their fp32 device tensors


def expand_grid(cfg: dict) -> list:
    """The reference's product (main.py:162-163): one dict per combination, scalars as one-element lists, in the order of
    ``itertools.product`` over the dict's key order."""
    keys = list(cfg)
    return [dict(zip(keys, combo)) for combo in product(*[v if isinstance(v, list) else [v] for v in cfg.values()])]


def load_grid(path) -> list:
    """``expand_grid`` of a YAML file of the reference's ``configs/``."""
    try:
        import yaml
    except ImportError as e:
        raise ImportError("gaussian.sweep.load_grid needs PyYAML to read a grid file; pass a dict to expand_grid instead") from e
    with open(path) as f:
        return expand_grid(yaml.safe_load(f))


def _full(point):
    return {**DEFAULTS, **point}


def make_data(point):
    """``(train, train2, val)``: the three ``generate_data`` calls of main.py:92-127 (seeds 42 / 44 / 43), cached by the keys they
    depend on: a grid over seeds x modes generates its data once."""
    p = _full(point)
    key = tuple(p[k] for k in _DATA_KEYS)
    hit = _DATA.get(key)
    if hit is None:
        base = dict(dim_c=p["data_dim_common"], dim_x=p["data_dim_x"], dim_y=p["data_dim_y"], dim_obs=p["dim_obs"],
                    noise_std=p["noise_std"], attenuation=p["attenuation"])
        hit = _DATA[key] = (
            generate_data(dict(base, seed=42, num_samples=p["train_num_samples"], attenuate_x=True, shared_latent_distribution_type="gaussian")),
            generate_data(dict(base, seed=44, num_samples=p["train_num_samples"], attenuate_x=True, shared_latent_distribution_type="laplace")),
            generate_data(dict(base, seed=43, num_samples=p["val_num_samples"], attenuate_x=False, shared_latent_distribution_type="gaussian")))
    return hit


def _device_data(point, device):
    """The tables of ``make_data(point)`` on ``device``, uploaded once: train x, train y, train2 y, val x, val y."""
    p = _full(point)
    key = (str(device),) + tuple(p[k] for k in _DATA_KEYS)
    hit = _DEVICE_DATA.get(key)
    if hit is None:
        train, train2, val = make_data(p)
        up = lambda t: t.to(device=device, dtype=torch.float32).contiguous()
        hit = _DEVICE_DATA[key] = dict(x=up(train["x"]), y=up(train["y"]), y2=up(train2["y"]), val_x=up(val["x"]), val_y=up(val["y"]))
    return hit


def build_point(point, device="cuda:0"):
    """``(dataset, generator, model, optimizer)`` of one grid point: ``build_run(fused=True)`` on ``make_data(point)``."""
    p = _full(point)
    train, train2, _ = make_data(p)
    return build_run(train, train2, mode=p["mode"], unrelated_info=bool(p["unrelated_info"]), train_num_samples=p["train_num_samples"],
                     batch_size=p["batch_size"], seed=p["seed"], dim_obs=p["dim_obs"], dim_common=p["dim_common"],
                     dim_latent=p["dim_latent"], lr=p["lr"], device=device, fused=True)


def sweep_grouped(points, *, num_steps=None, eval_every=1, alignment=False, group_size=None, device="cuda:0", on_done=None,
                  return_runs=False):
    """Runs the grid points in consecutive groups of ``group_size`` (default ``DEFAULT_GROUP_SIZE``) and returns one log per
    point, in grid order, with the keys and values ``train_model_steps_fused`` gives for that point alone.

    Per group: ``build_run(fused=True)`` per point in grid order, then the loop of ``train_model_steps_fused`` for all members
    at once: ``eval_every`` grouped steps (all of them when it is 0), one grouped evaluation forward, and with ``alignment`` the
    CKA and mutual k-NN (topk 10) of every member's validation embeddings.  All logs are read back once, at the end.
    ``num_steps`` overrides the points' own; without it the members of a group must agree on theirs.  ``on_done(point, model,
    log)`` is called per point, in grid order, after the read-back (checkpoints); ``return_runs=True`` returns ``(logs, runs)`` with
    one ``(model, optimizer)`` per point."""
    points = [dict(p) for p in points]
    group_size = DEFAULT_GROUP_SIZE if group_size is None else int(group_size)
    if group_size < 1:
        raise ValueError(f"sweep_grouped: group_size={group_size} < 1")
    if alignment:
        from umlh import align
    device = torch.device(device)
    pending = []        # (point, (model, optimizer), per-key device logs)
    for g0 in range(0, len(points), group_size):
        group = [_full(p) for p in points[g0:g0 + group_size]]
        steps = {int(p["num_steps"]) if num_steps is None else int(num_steps) for p in group}
        if len(steps) != 1:
            raise ValueError(f"sweep_grouped: the points {g0}..{g0 + len(group) - 1} disagree on num_steps {sorted(steps)}: pass num_steps")
        n = steps.pop()
        trainers, settings, val, models = [], [], [], []
        for p in group:
            ds, gen, model, opt = build_point(p, device)
            dev = _device_data(p, device)
            tables = (dev["x"], dev["y2"] if (p["mode"] != "xy" or p["unrelated_info"]) else dev["y"])
            trainers.append(FusedTrainer(model, opt, ds, p["batch_size"], gen, device, span_steps=min(max(n, 1), 4096), total_steps=n,
                                         tables=tables))
            settings.append((p["mode"], p["alpha_x"], p["alpha_y"]))
            val.append((dev["val_x"], dev["val_y"]))
            models.append((model, opt))
        grouped = GroupedTrainer(trainers, settings)
        logs = [{"loss": [], "val_loss_x": [], "val_loss_y": [], **({"val_cka": [], "val_mknn": []} if alignment else {})} for _ in group]
        step = 0
        while step < n:
            k = min(eval_every, n - step) if eval_every else n - step
            for log, losses in zip(logs, grouped.steps(k)):
                log["loss"].append(losses)
            step += k
            if eval_every and step % eval_every == 0:
                evals = grouped.evaluate(val, embeddings=alignment)
                for log, (v, _, _) in zip(logs, evals):
                    log["val_loss_x"].append(v[0]); log["val_loss_y"].append(v[1])
                if alignment:                                                 # main.py:78-84, all members in one call
                    res = align.measure_pairs([(ex, ey) for _, ex, ey in evals], topk=10)
                    for i, log in enumerate(logs):
                        log["val_cka"].append(res[i, 0]); log["val_mknn"].append(res[i, 4])
        pending.extend(zip(points[g0:g0 + group_size], models, logs))
    out = []
    for _, _, dlog in pending:                                                # the one read-back
        log = {"loss_x": [], "loss_y": [], "loss": [], "val_loss_x": [], "val_loss_y": []}
        if alignment:
            log.update(val_cka=[], val_mknn=[])
        if dlog["loss"]:
            host = torch.cat(dlog["loss"]).cpu()
            log["loss_x"], log["loss_y"], log["loss"] = ([float(t) for t in host[:, j]] for j in range(3))
        for k in ("val_loss_x", "val_loss_y", "val_cka", "val_mknn"):
            if k in log:
                log[k] = [float(t) for t in torch.stack(dlog[k]).cpu()] if dlog[k] else []
        out.append(log)
    if on_done is not None:
        for (point, run, _), log in zip(pending, out):
            on_done(point, run[0], log)
    return (out, [run for _, run, _ in pending]) if return_runs else out
