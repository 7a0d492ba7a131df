"""Training loop of the Gaussian experiment (reference Gaussian_experiment/main.py:33-91,132-151): infinite cycling
over one shuffled unpaired loader, ``loss = alpha_x*loss_x + alpha_y*loss_y`` ('xy') or ``loss_x`` ('x'), Adam through the
HIP optimizer kernel, validation reconstruction losses every ``eval_every`` steps.  With ``alignment=True`` every eval
also logs ``val_cka`` and ``val_mknn`` (topk 10) of the validation embeddings (main.py:78-84) through the HIP metric
kernels; they stay device scalars until the log is read back at the end.  wandb is outside the path."""
import torch
from torch.utils.data import DataLoader

from .data import UnpairedDataset, make_reproducible
from .model import SharedAutoencoder


def train_model_steps(model, data_loader, optimizer, num_steps, val_data_x, val_data_y, device, mode="xy", alpha_x=1.0,
                      alpha_y=1.0, eval_every=1, on_step=None, alignment=False):
    model.train()
    data_iter = iter(data_loader)
    log = {"loss_x": [], "loss_y": [], "loss": [], "val_loss_x": [], "val_loss_y": []}
    if alignment:
        from umlh import align
        log.update(val_cka=[], val_mknn=[])
    for step in range(num_steps):
        try:
            batch = next(data_iter)
        except StopIteration:
            data_iter = iter(data_loader)
            batch = next(data_iter)
        optimizer.zero_grad()
        x, y = batch["x"].to(device), batch["y"].to(device)
        loss_x, loss_y, _, _ = model(x, y)
        loss = alpha_x * loss_x + alpha_y * loss_y if mode == "xy" else loss_x
        loss.backward()
        optimizer.step()
        log["loss_x"].append(loss_x.detach()); log["loss_y"].append(loss_y.detach()); log["loss"].append(loss.detach())
        if eval_every and (step + 1) % eval_every == 0:
            model.eval()
            with torch.no_grad():
                vx, vy, _, _ = model(x=val_data_x, y=val_data_y)      # MSELoss(recon, data) of each view
                log["val_loss_x"].append(vx.detach()); log["val_loss_y"].append(vy.detach())
                if alignment:                                             # main.py:78-84
                    ex, ey = model.get_embeddings(val_data_x, val_data_y)
                    log["val_cka"].append(align.cka(ex, ey)); log["val_mknn"].append(align.mutual_knn(ex, ey, 10))
            model.train()
        if on_step is not None:
            on_step(step, loss_x, loss_y, loss)
    return {k: [float(t) for t in torch.stack(v).cpu()] if v else [] for k, v in log.items()}


def train_model_steps_fused(model, dataset, optimizer, num_steps, val_data_x, val_data_y, device, *, batch_size, generator, mode="xy",
                            alpha_x=1.0, alpha_y=1.0, eval_every=1, alignment=False):
    """``train_model_steps`` on the fused HIP step (``gaussian.fused.FusedTrainer``): the same batches as the reference's
    shuffled loader over ``dataset`` with ``generator``, ``eval_every`` steps per call (all of them when it is 0), one
    ``ae_forward`` on the validation tensors between calls.  Returns the same log dict, read back once at the end.  ``generator``
    is left where ``train_model_steps`` leaves the loader's after ``num_steps`` steps."""
    from .fused import FusedTrainer
    trainer = FusedTrainer(model, optimizer, dataset, batch_size, generator, device, span_steps=min(max(num_steps, 1), 4096), total_steps=num_steps)
    log = {"loss_x": [], "loss_y": [], "loss": [], "val_loss_x": [], "val_loss_y": []}
    if alignment:
        from umlh import align
        log.update(val_cka=[], val_mknn=[])
    vx = val_data_x.to(device=device, dtype=torch.float32)
    vy = val_data_y.to(device=device, dtype=torch.float32)
    losses = []
    step = 0
    while step < num_steps:
        k = min(eval_every, num_steps - step) if eval_every else num_steps - step
        losses.append(trainer.steps(k, mode=mode, alpha_x=alpha_x, alpha_y=alpha_y))
        step += k
        if eval_every and step % eval_every == 0:
            val, ex, ey = trainer.evaluate(vx, vy, embeddings=alignment)
            log["val_loss_x"].append(val[0]); log["val_loss_y"].append(val[1])
            if alignment:                                                 # main.py:78-84
                res = align.measure_pairs([(ex, ey)], topk=10)
                log["val_cka"].append(res[0, 0]); log["val_mknn"].append(res[0, 4])
    if losses:
        host = torch.cat(losses).cpu()
        log["loss_x"], log["loss_y"], log["loss"] = ([float(t) for t in host[:, j]] for j in range(3))
    for k in ("val_loss_x", "val_loss_y", "val_cka", "val_mknn"):
        if k in log:
            log[k] = [float(t) for t in torch.stack(log[k]).cpu()] if log[k] else []
    return log


def build_run(train_data, train_data2, *, mode="xy", unrelated_info=False, train_num_samples=10000, batch_size=512, seed=0,
              dim_obs=50, dim_common=128, dim_latent=10, lr=1e-3, device="cuda:0", fused=False):
    """Dataset / loader / model / optimizer wiring of main.py:132-148.  ``fused=True`` returns ``(dataset, generator, model,
    optimizer)`` for ``train_model_steps_fused`` instead of ``(loader, model, optimizer)``."""
    from engine.optimizer.optim import build_optimizer
    n = train_num_samples
    if mode == "xy":
        ysrc = train_data2 if unrelated_info else train_data
        ds = UnpairedDataset(train_data["x"][:n // 2], ysrc["y"][:n - n // 2])
    else:
        ds = UnpairedDataset(train_data["x"], train_data2["y"])
    g = torch.Generator()
    g.manual_seed(42)
    loader = DataLoader(ds, batch_size=batch_size, shuffle=True, drop_last=True, generator=g)
    make_reproducible(seed)
    model = SharedAutoencoder(dim_obs=dim_obs, dim_common=dim_common, dim_latent=dim_latent).to(device)
    if fused:
        return ds, g, model, build_optimizer(model.parameters(), "adam", lr, 0.0)
    return loader, model, build_optimizer(model.parameters(), "adam", lr, 0.0)
