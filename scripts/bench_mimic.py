#!/usr/bin/env python3
"""Time of the MIMIC loader (multibench/mimic.py; kernels of umlh_kernels_tabular.hip) on one GPU.

    python scripts/bench_mimic.py [--runs N] [--out profiles/mimic_bench.txt] [--skip-train]

A synthetic float64 ``im.pk`` dict of MIMIC's order of size: N = 36 000 samples, static [N, 5], series [N, 24, 12], batch 128.
  1. the table build (MimicTable: two uploads, two umlh_tab_standardize calls), wall clock around a synchronised build;
  2. the three kernels alone: ten launches enqueued back to back behind a fill between two device events, time / 10, median and
     range over ``--runs`` repetitions, and the achieved bytes/s, bytes = what a launch must move (standardize: the source
     three times -- two statistics passes and the apply -- and 4 written per element; perturb: 4 read, 4 written and the mask
     bytes per element; gather: 4 read and 4 written per word of a batch of 128).  The launches go through the Python
     wrappers: for the small kernels (perturb, gather) the figure is a floor of launch and enqueue cost, an upper bound of the
     kernel's time;
  3. the eleven noise levels of the test split through get_dataloader -- the host draws of all levels, which are timed alone
     as well, then per level the uploads and three launches -- against this script's own restatement of the reference's host
     loops in numpy on the CPU of the same machine WITHOUT the draws (one element or slice update per draw, as
     tabular_robust.py and timeseries_robust.py loop; the draws are the same host work on both sides);
  4. batches/s of one train epoch from the device loader against a torch DataLoader over the list of (static, series, label)
     tuples followed by the two uploads (num_workers = 0);
  5. ``train()`` for 100 batch pairs at z = 40 fed by the device loaders: ms per batch pair.
No threshold is fixed in advance: the file records every side measured in the same run."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda:0"
BACK_TO_BACK = 10
N, T_LEN, DT, DS, BATCH = 36000, 24, 12, 5, 128


def make_datafile(seed=0):
    g = np.random.default_rng(seed)
    xs = (g.standard_normal((N, DS)) + g.uniform(-4, 4, DS)) * g.uniform(0.5, 20.0, DS)
    xt = (g.standard_normal((N, T_LEN, DT)) + g.uniform(-4, 4, DT)) * g.uniform(0.1, 5.0, DT)
    xs[g.random(xs.shape) < 0.001] = np.nan
    xt[g.random(xt.shape) < 0.001] = np.inf
    return {"adm_features_all": xs, "ep_tdata": xt, "y_icd9": g.integers(0, 2, (N, 20)), "adm_labels_all": np.zeros((N, 6))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def spread(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def device_us(fn, runs, head):
    out = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        head.fill_(1)                                              # the launches queue behind this fill
        a.record()
        for _ in range(BACK_TO_BACK):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / BACK_TO_BACK)
    return out


def bench_kernels(table, runs):
    from umlh import seqload
    head = torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    res = {}
    src64 = torch.randn((N * T_LEN, DT), dtype=torch.float64, device=DEV, generator=g)
    src32 = src64.float()
    out = torch.empty_like(src32)
    for name, src, width in (("standardize_f64", src64, 8), ("standardize_f32", src32, 4)):
        fn = lambda: seqload.tab_standardize(src, out=out)
        fn()
        us = device_us(fn, runs, head)
        nbytes = src.numel() * (3 * width + 4)
        res[name] = {"shape": list(src.shape), "us": spread(us), "GB_per_s_at_median": round(nbytes / statistics.median(us) / 1e3, 1)}
    n_test = N // 5 - N // 10
    for name, x, with_carry in (("perturb_static", table.static[:n_test].contiguous(), True),
                                ("perturb_series_flat", table.series[:n_test].reshape(n_test, T_LEN * DT).contiguous(), False)):
        drop = (torch.rand(x.shape, device=DEV, generator=g) < 0.3).to(torch.uint8)
        carry = (torch.rand((x.shape[0], x.shape[1] - 1), device=DEV, generator=g) < 0.3).to(torch.uint8) if with_carry else None
        dst = torch.empty_like(x)
        fn = lambda: seqload.tab_perturb(x, drop, carry, out=dst)
        fn()
        us = device_us(fn, runs, head)
        nbytes = x.numel() * 9 + (0 if carry is None else carry.numel())
        res[name] = {"shape": list(x.shape), "us": spread(us), "GB_per_s_at_median": round(nbytes / statistics.median(us) / 1e3, 1)}
    ids = torch.randint(0, N, (BATCH,), device=DEV, generator=g)
    fn = lambda: seqload.rows_gather([table.static, table.series], ids)
    fn()
    us = device_us(fn, runs, head)
    res["rows_gather_batch_128"] = {"words": BATCH * (DS + T_LEN * DT), "us": spread(us),
                                    "GB_per_s_at_median": round(BATCH * (DS + T_LEN * DT) * 8 / statistics.median(us) / 1e3, 1)}
    return res


def host_levels(static, series, drawn):
    """The reference's loops restated: one element / slice update per draw."""
    for lv in drawn:
        st, se = static.copy(), series.copy()
        drop, carry = lv["drop"], lv["carry"]
        for i in range(len(st)):
            for j in range(DS):
                if drop[i, j]:
                    st[i][j] = 0
        for i in range(len(st)):
            for j in range(1, DS):
                if carry[i, j - 1]:
                    st[i][j] = st[i][j - 1]
        for i in range(len(se)):
            se[i] += lv["eps"][i]
        flat = se.reshape(len(se), -1)
        for i in range(len(se)):
            row, mask = flat[i], lv["elem"][i]
            for j in np.flatnonzero(mask):                         # the reference tests every element; this visits the hits only
                row[j] = 0
        for i in range(len(se)):
            if not lv["keep"][i]:
                se[i] = np.zeros(se[i].shape)


def bench_levels(table, runs):
    from multibench.mimic import draw_mimic_noise, get_dataloader
    n_test = len(table.test)
    t_draw, drawn = wall(lambda: draw_mimic_noise(n_test, rng=1))

    def device():
        _, _, tests = get_dataloader(7, 40, table=table, rng=1)
        for k in range(11):
            tests["timeseries"].tables(k)
    dev = [wall(device)[0] * 1e3 for _ in range(runs)]
    static = table.static[torch.tensor(table.test, device=DEV)].double().cpu().numpy()
    series = table.series[torch.tensor(table.test, device=DEV)].double().cpu().numpy()
    t0 = time.perf_counter()
    host_levels(static, series, drawn)
    host = (time.perf_counter() - t0) * 1e3
    return {"test_samples": n_test, "device_11_levels_with_draws_ms": spread(dev), "draws_alone_ms": round(t_draw * 1e3, 1),
            "host_loops_numpy_11_levels_without_draws_ms": round(host, 1)}


def bench_batches(table, runs):
    from multibench.mimic import get_dataloader
    trains, _, _ = get_dataloader(7, BATCH, table=table, generator=torch.Generator().manual_seed(1), tabular_robust=False,
                                  timeseries_robust=False)

    def device_epoch():
        k = 0
        for _ in trains:
            k += 1
        return k
    dev = []
    for _ in range(runs):
        t, k = wall(device_epoch)
        dev.append(k / t)
    static, series = table.static.double().cpu().numpy(), table.series.double().cpu().numpy()
    data = [(static[i], series[i], table.labels[i]) for i in table.train]
    loader = torch.utils.data.DataLoader(data, shuffle=True, num_workers=0, batch_size=BATCH)

    def host_epoch():
        k = 0
        for st, se, _ in loader:
            st.float().to(DEV), se.float().to(DEV)
            k += 1
        return k
    host = []
    for _ in range(max(1, runs // 2)):
        t, k = wall(host_epoch)
        host.append(k / t)
    return {"batches_per_epoch": len(trains), "device_loader_batches_per_s": spread(dev, 0), "torch_dataloader_plus_h2d_batches_per_s": spread(host, 0)}


def bench_train(datafile, pairs=100):
    from multibench.mimic import build_run
    from multibench.train import train
    torch.manual_seed(0)
    run = build_run(datafile, 40, generator=torch.Generator().manual_seed(1), generator_2=torch.Generator().manual_seed(2), device=DEV)

    class First:
        def __init__(self, loader, k):
            self.loader, self.k = loader, k

        def __iter__(self):
            for i, b in enumerate(self.loader):
                if i >= self.k:
                    return
                yield b
    l1, l2 = First(run["train_loader"], pairs), First(run["train_loader_2"], pairs)
    train(run["model"], "xy", First(run["train_loader"], 5), First(run["train_loader_2"], 5), run["optimizer"], num_epoch=1, step_k=-1,
          ds_name=run["ds_name"], device=DEV)
    t, res = wall(lambda: train(run["model"], "xy", l1, l2, run["optimizer"], num_epoch=1, step_k=-1, ds_name=run["ds_name"], device=DEV))
    return {"z": 40, "batch_pairs": len(res["loss"]), "ms_per_batch_pair": round(t * 1e3 / len(res["loss"]), 3), "last_loss": res["loss"][-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mimic_bench.txt"))
    ap.add_argument("--skip-train", action="store_true")
    args = ap.parse_args()
    from multibench.mimic import MimicTable
    datafile = make_datafile()
    MimicTable(datafile, 7, DEV)                                   # warm-up: library load, allocator
    builds = []
    for _ in range(args.runs):
        t, table = wall(lambda: MimicTable(datafile, 7, DEV))
        builds.append(t * 1e3)
    lines = [f"device: {torch.cuda.get_device_name(0)}; host threads {torch.get_num_threads()}",
             "note: kernel times are device events around ten back-to-back launches / 10, median and range over the runs; everything "
             "else is wall clock around synchronised work",
             json.dumps({"table_build": {"shape": [N, T_LEN, DT, DS], "source": "float64", "ms": spread(builds)}}),
             json.dumps({"kernels": bench_kernels(table, args.runs)}),
             json.dumps({"noise_levels": bench_levels(table, args.runs)}),
             json.dumps({"batches": bench_batches(table, args.runs)})]
    if not args.skip_train:
        lines.append(json.dumps({"train": bench_train(datafile)}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
