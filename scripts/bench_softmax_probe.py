"""Timings of the multinomial logistic probe (umlh.SoftmaxProbe, finetune.linear_probe) -> profiles/softmax_probe_bench.txt.

Per size: the HIP fit (time and iterations at gtol = 1e-4 n, max_iter = 200), one evaluation of (f, g) with the FLOP/s its two
GEMMs reach when the whole evaluation is charged to them (a lower bound), the same L-BFGS written in torch ops on the same GPU
(two-loop recursion on device vectors, Armijo backtracking with a host read per trial), and sklearn's
LogisticRegression(max_iter=200) on the CPU where it imports (the largest size only with --sklearn-large: it takes minutes).
Then one whole finetune.linear_probe over the five-point C grid with and without warm starts.

    python scripts/bench_softmax_probe.py [--reps 3] [--no-sklearn] [--sklearn-large] [--out profiles/softmax_probe_bench.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "unpaired-multimodal-learning_amd")]
import umlh  # noqa: E402

DEV = "cuda:0"
SIZES = [("few-shot 16/class", 1600, 512, 100), ("16 000 x 1024, 1000 classes", 16000, 1024, 1000), ("MOSEI size", 16265, 600, 7)]


def blobs(n, d, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    centers = torch.randn(k, d, generator=g) * (2.0 / d ** 0.5)
    y = torch.arange(n) % k
    y = y[torch.randperm(n, generator=g)]
    x = centers[y] + torch.randn(n, d, generator=g) * (1.5 / d ** 0.5)
    return x.to(DEV), y.to(DEV)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), out


def torch_lbfgs(x, y, k, c=1.0, max_iter=200, history=10, gtol=None):
    """The same objective and the same kind of iteration in torch ops: fp32 logits, two-loop recursion, Armijo backtracking."""
    n, d = x.shape
    gtol = 1e-4 * n if gtol is None else gtol
    xt = torch.cat([x, torch.ones(n, 1, device=x.device)], 1)
    onehot = torch.nn.functional.one_hot(y, k).float()
    pen = torch.ones(1, d + 1, device=x.device)
    pen[0, d] = 0

    def fg(w):
        z = xt @ w.T
        lse = torch.logsumexp(z.double(), 1)
        f = (lse - z.double().gather(1, y[:, None])[:, 0]).sum() + 0.5 / c * (w * pen).double().pow(2).sum()
        r = torch.softmax(z, 1) - onehot
        return f, r.T @ xt + w * pen / c

    w = torch.zeros(k, d + 1, device=x.device)
    f, g = fg(w)
    S, Y, it = [], [], 0
    while it < max_iter and float(g.abs().max()) > gtol:
        q = g.clone()
        al = []
        for s, yv in zip(reversed(S), reversed(Y)):
            a = (s * q).sum() / (s * yv).sum()
            q -= a * yv
            al.append(a)
        if S:
            q *= (S[-1] * Y[-1]).sum() / (Y[-1] * Y[-1]).sum()
        else:
            q /= g.abs().sum()
        for (s, yv), a in zip(zip(S, Y), reversed(al)):
            q += (a - (yv * q).sum() / (s * yv).sum()) * s
        p, gtp, t = -q, -(g * q).sum().double(), 1.0
        while t > 2.0 ** -12:
            fn, gn = fg(w + t * p)
            if float(fn) <= float(f + 1e-4 * t * gtp):
                break
            t *= 0.5
        else:
            break
        S.append(t * p)
        Y.append(gn - g)
        S, Y = S[-history:], Y[-history:]
        w, f, g, it = w + t * p, fn, gn, it + 1
    return w, it, float(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-sklearn", action="store_true")
    ap.add_argument("--sklearn-large", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_probe_bench.txt"))
    a = ap.parse_args()
    lines = [f"softmax probe on {torch.cuda.get_device_name(0)} (min of {a.reps} runs after one warm-up; gtol = 1e-4 n, max_iter = 200, C = 1)"]
    from umlh._lib import check, load_library
    lib = load_library()
    for tag, n, d, k in SIZES:
        x, y = blobs(n, d, k)
        t_fit, pr = timed(lambda: umlh.SoftmaxProbe().fit(x, y, check_classes=False, n_classes=k), a.reps)
        rec = pr.record()
        nbytes = lib.umlh_softmax_probe_scratch_bytes(n, d, k, 0, 1)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = torch.empty(2, dtype=torch.float64, device=DEV)
        coef = torch.cat([pr.coef_, pr.intercept_[:, None]], 1).contiguous()
        y32 = y.to(torch.int32)

        def ev():
            check(lib.umlh_softmax_probe_eval(x.data_ptr(), n, d, d, y32.data_ptr(), None, k, 1.0, coef.data_ptr(), d + 1, out.data_ptr(), None,
                                              0, out[1:].data_ptr(), scratch.data_ptr(), nbytes, None), "eval")
        with torch.cuda.stream(torch.cuda.default_stream()):
            t_ev, _ = timed(ev, a.reps)
        flops = 2.0 * 2.0 * n * k * (d + 1)
        t_torch, (_, it_t, f_t) = timed(lambda: torch_lbfgs(x, y, k), 1)
        lines.append(f"{tag}: n={n} d={d} classes={k}")
        lines.append(f"  HIP fit         {t_fit * 1e3:9.2f} ms  iterations {rec['n_iter']:3d}  converged {rec['converged']}  objective {rec['objective']:.8g}  "
                     f"({t_fit * 1e3 / max(rec['n_iter'], 1):.3f} ms / iteration)")
        lines.append(f"  HIP (f, g) eval {t_ev * 1e3:9.3f} ms  two GEMMs = {flops / 1e9:.2f} GFLOP -> at least {flops / t_ev / 1e12:.2f} TFLOP/s")
        lines.append(f"  torch-op L-BFGS {t_torch * 1e3:9.2f} ms  iterations {it_t:3d}  objective {f_t:.8g}")
        if not a.no_sklearn and (n * d * k < 1e9 or a.sklearn_large):
            try:
                from sklearn.linear_model import LogisticRegression
                xc, yc = x.cpu().numpy().astype(np.float64), y.cpu().numpy()
                t0 = time.perf_counter()
                import warnings
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    sk = LogisticRegression(max_iter=200).fit(xc, yc)
                lines.append(f"  sklearn (CPU)   {(time.perf_counter() - t0) * 1e3:9.2f} ms  iterations {int(sk.n_iter_[0]):3d}")
            except ImportError:
                lines.append("  sklearn (CPU)   not installed")
        elif not a.no_sklearn:
            lines.append("  sklearn (CPU)   not run at this size (minutes; --sklearn-large)")
        print("\n".join(lines[-5:]), flush=True)
    import finetune
    x, y = blobs(1600, 512, 100, seed=1)
    xc, yc = x.cpu(), y.cpu()
    split = [(xc[s], yc[s]) for s in (slice(0, 960), slice(960, 1280), slice(1280, 1600))]
    for warm in (True, False):
        t, out = timed(lambda: finetune.linear_probe(*split, num_classes=100, device=DEV, warm_start=warm), a.reps)
        lines.append(f"linear_probe, 5-point C grid, 960/320/320 x 512, 100 classes, warm_start={warm}: {t * 1e3:.2f} ms  iterations "
                     f"{[r['n_iter'] for r in out['records']]}  best C {out['best_C']}  val {out['val_acc']:.4f}  test {out['test_acc']:.4f}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
