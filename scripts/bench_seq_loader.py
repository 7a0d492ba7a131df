#!/usr/bin/env python3
"""Time of the affect datasets' device loader (multibench/data.py, umlh_kernels_seqload.hip) against the host form on the same
machine.

    python scripts/bench_seq_loader.py [--runs N] [--pairs P] [--out profiles/seq_loader_bench.txt]

Synthetic fp32 splits at 16 265 x 50 x 35/74/300 with batch 32 (MOSEI) and at 8 000 x 50 x 371/81/300 with batch 128 (sarcasm /
humor with vision_norm), front-padded with zeros to random lengths.  Per shape:
  1. table build time (upload, first-row kernel, one read-back, normalisation): wall clock around a synchronised build;
  2. batches/s of the device loader alone over one shuffled epoch (wall clock, synchronised at the end);
  3. the gather-pad kernel alone, for every batch of an epoch: ten launches of the same batch enqueued back to back behind a
     0.5 ms fill (so that all ten are queued before the first may start) between two device events, time / 10, and the achieved
     bytes/s, bytes = what a launch must read and write (4 * copied words read, 4 * block words written, 8 * b lengths,
     8 * b ids, 4 * b starts);
  4. the host form: this script's own restatement of the reference loader's work -- per sample three torch.tensor copies, a
     nonzero, three slices and .float(), then pad_sequence per modality -- behind a torch DataLoader with num_workers 0 and 2,
     plus the host-to-device copies of the two modalities the step uses; batches/s over one epoch;
  5. multibench.train.train for ``--pairs`` batch pairs (z = 40, the alternation step of scripts/bench_multibench.py) fed by
     two device loaders and fed by two host-form loaders (num_workers 0 and 2), ms per batch pair, alternating.
No threshold is fixed in advance: the file records both sides measured in the same run."""
import argparse
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd"), os.path.join(ROOT, "scripts")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.nn.utils.rnn import pad_sequence  # noqa: E402

DEV = "cuda:0"
BACK_TO_BACK = 10
SHAPES = {"mosei": (16265, 50, (35, 74, 300), 32, False), "sarcasm": (8000, 50, (371, 81, 300), 128, True)}


def make_split(n, T, dims, seed):
    g = np.random.default_rng(seed)
    start = g.integers(0, T - 4, n)
    front = np.arange(T)[None, :, None] < start[:, None, None]
    split = {k: np.where(front, np.float32(0), g.standard_normal((n, T, d), dtype=np.float32)) for k, d in zip(("vision", "audio", "text"), dims)}
    split["text"][np.arange(n), start, 0] = 1.0
    split["labels"] = g.standard_normal((n, 1, 1), dtype=np.float32)
    split["id"] = np.arange(n).reshape(n, 1)
    return split


class HostDataset(torch.utils.data.Dataset):
    """The per-sample work of the reference's Dataset (trim by the first nonzero text row), restated."""

    def __init__(self, split):
        self.s = split

    def __len__(self):
        return self.s["text"].shape[0]

    def __getitem__(self, i):
        v, a, t = (torch.tensor(self.s[k][i]) for k in ("vision", "audio", "text"))
        start = t.nonzero(as_tuple=False)[0][0]
        return [v[start:].float(), a[start:].float(), t[start:].float(), i, torch.tensor(self.s["labels"][i]).float()]


def host_collate(samples):
    xs, ls = [], []
    for m in range(3):
        seqs = [s[m] for s in samples]
        ls.append(torch.as_tensor([q.size(0) for q in seqs]))
        xs.append(pad_sequence(seqs, batch_first=True))
    return xs, ls, torch.tensor([s[3] for s in samples]).view(-1, 1), torch.tensor([s[4] for s in samples]).view(-1, 1)


def host_loader(split, bs, workers):
    return torch.utils.data.DataLoader(HostDataset(split), batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(42),
                                       num_workers=workers, collate_fn=host_collate)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def bench_shape(name, runs, pairs):
    from bench_multibench import build
    from engine.optimizer.optim import build_optimizer
    from multibench.data import AffectTable, SequenceLoader
    from multibench.train import train
    from umlh import seqload
    n, T, dims, bs, vnorm = SHAPES[name]
    split = make_split(n, T, dims, 5)
    res = {"shape": name, "n": n, "T": T, "dims": dims, "batch_size": bs, "vision_norm": vnorm}
    AffectTable(make_split(64, T, dims, 6), vision_norm=vnorm, device=DEV)                  # warm-up: code objects, allocator
    builds = [wall(lambda: AffectTable(split, vision_norm=vnorm, device=DEV)) for _ in range(runs)]
    table = builds[-1][1]
    res["table_build_ms"] = [round(t * 1e3, 2) for t, _ in builds]
    mk = lambda mods=(0, 1, 2): SequenceLoader(table, bs, shuffle=True, generator=torch.Generator().manual_seed(42), modalities=mods)

    def epoch(loader):
        k = 0
        for _ in loader:
            k += 1
        return k
    epoch(mk())
    t = [wall(lambda: epoch(mk())) for _ in range(runs)]
    res["device_loader_batches_per_s"] = [round(k / s, 1) for s, k in t]
    # the kernel alone, every batch of one epoch: BACK_TO_BACK launches between two device events, queued behind a long fill
    order = torch.randperm(len(table), generator=torch.Generator().manual_seed(1))
    order_dev = order.to(DEV)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(0, len(table), bs)]
    head = torch.empty(1 << 30, dtype=torch.uint8, device=DEV)                              # the fill the launches queue behind
    for rep in range(2):                                                                     # the first pass warms up
        total_bytes = 0
        for (e0, e1), lo in zip(ev, range(0, len(table), bs)):
            ids = order[lo:lo + bs].numpy()
            t_out = int(table.lengths[ids].max())
            outs = [torch.empty((len(ids), t_out, d), dtype=torch.float32, device=DEV) for d in dims]
            lens = torch.empty(len(ids), dtype=torch.int64, device=DEV)
            head.zero_()
            e0.record()
            for _ in range(BACK_TO_BACK):
                seqload.gather_pad(table.tables, table.start, order_dev[lo:lo + bs], t_out, outs=outs, lengths=lens)
            e1.record()
            total_bytes += 4 * int(table.lengths[ids].sum()) * sum(dims) + 4 * len(ids) * t_out * sum(dims) + 20 * len(ids)
        torch.cuda.synchronize()
    del head
    us = [a.elapsed_time(b) * 1e3 / BACK_TO_BACK for a, b in ev]
    res["gather_pad_kernel"] = {"launches": len(us), "median_us": round(statistics.median(us), 2), "min_us": round(min(us), 2),
                                "max_us": round(max(us), 2), "bytes_per_launch_mean": total_bytes // len(us),
                                "achieved_GB_per_s": round(total_bytes / (sum(us) * 1e-6) / 1e9, 1)}
    # the host form
    for workers in (0, 2):
        def host_epoch():
            k = 0
            for xs, ls, _, _ in itertools.islice(host_loader(split, bs, workers), pairs):
                xs[0].to(DEV), xs[2].to(DEV), ls[0].to(DEV), ls[2].to(DEV)
                k += 1
            return k
        host_epoch()
        t = [wall(host_epoch) for _ in range(runs)]
        res[f"host_form_workers_{workers}_batches_per_s"] = [round(k / s, 1) for s, k in t]
    # train() fed by either
    torch.manual_seed(0)
    model = build(40, dims[0], dims[2])
    opt = build_optimizer(model.parameters(), "adam", 1e-3, 0.0)

    def run(l1, l2):
        s, _ = wall(lambda: train(model, "xy", itertools.islice(l1, pairs), itertools.islice(l2, pairs), opt, num_epoch=1, step_k=-1,
                                  ds_name="mosei", device=DEV))
        return s * 1e3 / pairs
    feeds = {"device_loaders": lambda: (mk((0, 2)), mk((0, 2))),
             "host_form_workers_0": lambda: (host_loader(split, bs, 0), host_loader(split, bs, 0)),
             "host_form_workers_2": lambda: (host_loader(split, bs, 2), host_loader(split, bs, 2))}
    for f in feeds.values():
        run(*f())
    t = {k: [] for k in feeds}
    for _ in range(runs):
        for k, f in feeds.items():
            t[k].append(round(run(*f()), 3))
    res["train_ms_per_batch_pair"] = {k: {"runs": v, "median": statistics.median(v)} for k, v in t.items()}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=100)
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seq_loader_bench.txt"))
    args = ap.parse_args()
    lines = [f"device: {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}",
             f"note: the host-form and train() figures are runs of {args.pairs} batches (batch pairs); a host-form loader is made anew per run, as the "
             "reference makes its iterators per epoch, so with num_workers=2 the start of the worker processes is inside the figure"]
    for name in args.shapes:
        lines.append(json.dumps(bench_shape(name, args.runs, args.pairs)))
        print(lines[-1], flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
