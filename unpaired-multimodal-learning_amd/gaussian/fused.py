"""The fused training path of the Gaussian experiment: the batch order of the reference's shuffled loader restated on the
host, and a trainer that runs whole steps of the SharedAutoencoder through ``umlh.gauss.ae_train_steps`` (two launches per
step) with the batches gathered by index from device-resident tables; ``GroupedTrainer`` steps several such trainers in one
launch pair per step (``umlh.gauss.ae_train_steps_grouped``).

``BatchOrder`` reproduces, draw for draw, the index stream of
``DataLoader(UnpairedDataset, batch_size, shuffle=True, drop_last=True, generator=g)`` cycled by ``train_model_steps``'
``StopIteration`` restart.  Per epoch the loader draws its iterator's base seed
(``torch.empty((), dtype=int64).random_(generator=g)``), then ``randperm(n)``, yields ``n // batch_size`` batches, and -- when
the next batch is asked for -- ALWAYS makes one more ``randperm(n)`` draw whose values are unused (the sampler's tail
``randperm(n)[:num_samples % n]``), whether or not ``batch_size`` divides ``n``."""
from __future__ import annotations

import torch


class BatchOrder:
    """The int64 host index stream of the reference's loader; ``take(k)`` returns the next ``k * batch_size`` dataset indices.
    Two consecutive ``take`` calls give what one long call gives."""

    def __init__(self, n, batch_size, generator):
        n, batch_size = int(n), int(batch_size)
        if batch_size < 1:
            raise ValueError(f"batch_order: batch_size={batch_size} < 1")
        if n < batch_size:
            raise ValueError(f"batch_order: n={n} < batch_size={batch_size}: the reference's loader yields no batch (an endless loop there)")
        self.n, self.batch_size, self.generator = n, batch_size, generator
        self._perm = None
        self._next = 0              # next batch of the epoch

    def _epoch(self):
        g = self.generator
        if self._perm is not None:
            torch.randperm(self.n, generator=g)                          # the sampler's unused tail draw
        torch.empty((), dtype=torch.int64).random_(generator=g)           # the iterator's base seed
        self._perm = torch.randperm(self.n, generator=g)
        self._next = 0

    def take(self, num_steps):
        num_steps = int(num_steps)
        out = torch.empty(num_steps * self.batch_size, dtype=torch.int64)
        per_epoch = self.n // self.batch_size
        done = 0
        while done < num_steps:
            if self._perm is None or self._next == per_epoch:
                self._epoch()
            k = min(num_steps - done, per_epoch - self._next)
            lo = self._next * self.batch_size
            out[done * self.batch_size:(done + k) * self.batch_size] = self._perm[lo:lo + k * self.batch_size]
            self._next += k
            done += k
        return out


def batch_order(n, batch_size, generator, num_steps):
    """The first ``num_steps`` batches (``num_steps * batch_size`` int64 dataset indices) of a fresh loader over ``n`` samples."""
    return BatchOrder(n, batch_size, generator).take(num_steps)


class FusedTrainer:
    """Fused steps of ``model`` (a ``gaussian.model.SharedAutoencoder`` on ``device``) over ``dataset`` (an ``UnpairedDataset``).

    The two tables are uploaded once; the row ids of a span of steps are built on the host (``BatchOrder``, ids
    ``order % len_x`` and ``order % len_y`` as ``UnpairedDataset.__getitem__``) and uploaded as two int32 tables.  The kernels
    update the model's parameters and the optimizer's ``state_for(p)`` tensors through their own storages, so ``state_dict``,
    checkpoints and a later ``optimizer.step()`` keep working."""

    def __init__(self, model, optimizer, dataset, batch_size, generator, device, span_steps=1024, total_steps=None, tables=None):
        self.model, self.optimizer, self.device = model, optimizer, torch.device(device)
        self.batch_size = int(batch_size)
        self.order = BatchOrder(len(dataset), batch_size, generator)
        self.len_x, self.len_y = dataset.len_x, dataset.len_y
        # tables: (x, y) fp32 device tensors that already hold the dataset's rows (row i of the view at row i): used as they
        # are, so that trainers over the same data share one upload
        if tables is None:
            tables = (torch.as_tensor(dataset.data_x).to(self.device, torch.float32).contiguous(),
                      torch.as_tensor(dataset.data_y).to(self.device, torch.float32).contiguous())
        self.x, self.y = tables
        for t, rows, name in ((self.x, self.len_x, "x"), (self.y, self.len_y, "y")):
            if t.device != self.device or t.dtype != torch.float32 or t.ndim != 2 or t.shape[0] < rows:
                raise ValueError(f"FusedTrainer: tables[{name}] must be an fp32 device tensor of at least {rows} rows on {self.device}")
        self.span_steps = max(int(span_steps), 1)
        # the row ids of a span are drawn ahead of the steps that use them.  total_steps (the steps the caller will run in all)
        # caps what is drawn, so that the generator ends where the reference's loader leaves it after that many steps; without
        # it the generator may be up to span_steps - 1 steps ahead of the steps run
        self.total_steps = None if total_steps is None else int(total_steps)
        self._drawn = 0
        self.params = [p for _, p in model.named_parameters()]
        known = {id(p) for p in optimizer.param_groups[0]["params"]}
        if any(id(p) not in known for p in self.params):
            raise ValueError("FusedTrainer: the optimizer does not hold the model's parameters")
        sgd = optimizer.name == "sgd"
        st = [optimizer.state_for(p) for p in self.params]
        self.m = [s["momentum_buffer" if sgd else "exp_avg"] for s in st]
        self.v = None if sgd else [s["exp_avg_sq"] for s in st]
        self._idx_x = self._idx_y = None
        self._have = self._used = 0

    def _refill(self, need):
        steps = max(need, self.span_steps)
        if self.total_steps is not None:
            steps = max(need, min(steps, self.total_steps - self._drawn))
        self._drawn += steps
        order = self.order.take(steps)
        self._idx_x = (order % self.len_x).to(torch.int32).to(self.device)
        self._idx_y = (order % self.len_y).to(torch.int32).to(self.device)
        self._have, self._used = steps, 0

    def _step_args(self, k, mode, alpha_x, alpha_y, losses):
        """The arguments of ``ae_train_steps`` (``n_steps`` excepted) for the next ``k`` steps of the current id span."""
        g = self.optimizer.param_groups[0]
        b = self.batch_size
        lo, hi = self._used * b, (self._used + k) * b
        return dict(params=[p.data for p in self.params], m=self.m, v=self.v, x=self.x, y=self.y, idx_x=self._idx_x[lo:hi],
                    idx_y=self._idx_y[lo:hi], batch_x=b, batch_y=b, mode=mode, alpha_x=alpha_x, alpha_y=alpha_y,
                    optimizer=self.optimizer.name, lr=g["lr"], first_step=self.optimizer.step_count + 1, betas=g["betas"], eps=g["eps"],
                    momentum=g["momentum"], weight_decay=g["weight_decay"], losses=losses)

    def steps(self, n, mode="xy", alpha_x=1.0, alpha_y=1.0):
        """Runs ``n`` steps; returns their [n, 3] device losses (loss_x, loss_y, loss) and advances ``optimizer.step_count``."""
        from umlh import gauss
        n = int(n)
        out = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        done = 0
        while done < n:
            if self._used == self._have:
                self._refill(min(n - done, 65536))
            k = min(n - done, self._have - self._used, 65536)
            gauss.ae_train_steps(n_steps=k, **self._step_args(k, mode, alpha_x, alpha_y, out[done:done + k]))
            self.optimizer.step_count += k
            self._used += k
            done += k
        return out

    def evaluate(self, val_x, val_y, embeddings=False):
        """``(losses [2], emb_x, emb_y)`` of one ``ae_forward`` on the validation tensors."""
        from umlh import gauss
        losses, _, _, ex, ey = gauss.ae_forward([p.data for p in self.params], val_x, val_y, recon=False, embeddings=embeddings)
        return losses, ex, ey


class GroupedTrainer:
    """Several ``FusedTrainer``s stepped together through ``umlh.gauss.ae_train_steps_grouped``: two launches per step for the
    whole group.  The members' tables, id spans, bound parameters and moments are used as they are, and every member is left --
    parameters, moments, ``optimizer.step_count``, generator -- exactly where its own ``FusedTrainer.steps`` would leave it.
    ``settings``: one ``(mode, alpha_x, alpha_y)`` per member."""

    def __init__(self, trainers, settings):
        self.trainers, self.settings = list(trainers), [tuple(s) for s in settings]
        if not self.trainers or len(self.trainers) != len(self.settings):
            raise ValueError("GroupedTrainer: one (mode, alpha_x, alpha_y) per trainer, at least one trainer")
        self.device = self.trainers[0].device
        if any(t.device != self.device for t in self.trainers):
            raise ValueError("GroupedTrainer: the members live on different devices")

    def steps(self, n):
        """Runs ``n`` steps of every member; returns the members' [n, 3] device losses.  The call is split where any member's id
        span runs out; that member refills as it would alone."""
        from umlh import gauss
        n = int(n)
        outs = [torch.empty((n, 3), dtype=torch.float32, device=self.device) for _ in self.trainers]
        done = 0
        while done < n:
            for t in self.trainers:
                if t._used == t._have:
                    t._refill(min(n - done, 65536))
            k = min([n - done, 65536] + [t._have - t._used for t in self.trainers])
            gauss.ae_train_steps_grouped([t._step_args(k, mode, ax, ay, out[done:done + k])
                                          for t, (mode, ax, ay), out in zip(self.trainers, self.settings, outs)], k)
            for t in self.trainers:
                t.optimizer.step_count += k
                t._used += k
            done += k
        return outs

    def evaluate(self, val, embeddings=False):
        """One grouped forward over all members.  ``val``: one ``(val_x, val_y)`` pair of device tensors per member (members may
        name the same tensors).  Returns one ``(losses [2], emb_x, emb_y)`` per member."""
        from umlh import gauss
        out = gauss.ae_forward_grouped([dict(params=[p.data for p in t.params], x=vx, y=vy, recon=False, embeddings=embeddings)
                                        for t, (vx, vy) in zip(self.trainers, val)])
        return [(losses, ex, ey) for losses, _, _, ex, ey in out]
