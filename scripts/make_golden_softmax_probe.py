"""Writes tests/golden/softmax_probe*.npz: the fixtures of the multinomial logistic probe.  CPU only (numpy, scipy, sklearn).

The inputs are not stored: tests/_softmax_probe_ref.py: make_case regenerates them from the case's seed, and the fixture pins a
checksum of the regenerated arrays.  Per case the fixture holds
    <case>.x_sum / <case>.y_sum      sha256 prefixes of the fp32 features and int32 labels (as uint8 arrays)
    <case>.sk_coef / .sk_intercept / .sk_n_iter   sklearn's LogisticRegression(max_iter=200, C=1) on the float64 copy of the fp32
                                     features the kernels see (standardised for the `std` case)
    <case>.opt                       the float64 optimum [K, d + 1] of the sum objective: scipy L-BFGS-B, maxcor=30, ftol=1e-16,
                                     gtol=1e-9
    <case>.tau                       8 x the largest logit error of the fp32 restatement of the device algorithm against the
                                     float64 optimum's logits, rounded up to a power of two
Files stay below 1 MB: the arrays of the large case go to .partN files (tests/conftest.py: load_golden merges them).
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _softmax_probe_ref as R  # noqa: E402


def optimum(xt, y, K, C):
    from scipy.optimize import minimize
    D = xt.shape[1]

    def fg(w):
        f, g = R.objective_grad(w.reshape(K, D), xt, y, C)
        return f, g.ravel()

    res = minimize(fg, np.zeros(K * D), jac=True, method="L-BFGS-B",
                   options=dict(maxcor=30, ftol=1e-16, gtol=1e-9, maxiter=20000, maxfun=40000))
    return res.x.reshape(K, D)


def main():
    from sklearn.linear_model import LogisticRegression
    out = os.path.join(ROOT, "tests", "golden")
    small, parts = {}, []
    for name, c in R.CASES.items():
        x, y = R.make_case(name)
        stats = R.column_stats(x) if c["standardize"] else None
        xt = R.x_tilde(x, stats)
        K, d = c["K"], c["d"]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = LogisticRegression(max_iter=200, C=R.C_REG).fit(xt[:, :d].astype(np.float64), y)
        opt = optimum(xt, y, K, R.C_REG)
        f_opt, g_opt = R.objective_grad(opt, xt, y, R.C_REG)
        f_sk, _ = R.objective_grad(np.concatenate([sk.coef_, sk.intercept_[:, None]], 1), xt, y, R.C_REG)
        fit = R.fit_fp32(x, y, C=R.C_REG, stats=stats, gtol=1e-6 * c["n"])
        f_fit, g_fit = R.objective_grad(fit["W"], xt, y, R.C_REG)
        zerr = np.abs(xt.astype(np.float64) @ (fit["W"].astype(np.float64) - opt).T).max()
        tau = R.pow2_ceil(8.0 * zerr)
        _, marg = R.margins(opt, xt)
        print(f"{name}: f_opt={f_opt:.10g} max|g_opt|={np.abs(g_opt).max():.2e}  sklearn gap={(f_sk - f_opt) / f_opt:.2e} n_iter={int(sk.n_iter_[0])}"
              f"  fp32 fit: conv={fit['converged']} it={fit['n_iter']} gap={(f_fit - f_opt) / f_opt:.2e} max|g|={np.abs(g_fit).max():.2e}"
              f"  zerr={zerr:.2e} tau={tau:.3g} undecidable={np.mean(marg <= tau):.4f}")
        arrs = {f"{name}.x_sum": np.frombuffer(R.checksum(x).encode(), np.uint8),
                f"{name}.y_sum": np.frombuffer(R.checksum(y).encode(), np.uint8),
                f"{name}.sk_coef": sk.coef_.astype(np.float64), f"{name}.sk_intercept": sk.intercept_.astype(np.float64),
                f"{name}.sk_n_iter": np.asarray(sk.n_iter_, np.int64), f"{name}.opt": opt, f"{name}.tau": np.float64(tau)}
        if K * (d + 1) * 8 > 300_000:
            parts.append({f"{name}.opt": arrs.pop(f"{name}.opt")})
            parts.append({f"{name}.sk_coef": arrs.pop(f"{name}.sk_coef")})
        small.update(arrs)
    np.savez_compressed(os.path.join(out, "softmax_probe.npz"), **small)
    for i, p in enumerate(parts, 1):
        np.savez_compressed(os.path.join(out, f"softmax_probe.part{i}.npz"), **p)
    for fn in sorted(os.listdir(out)):
        if fn.startswith("softmax_probe"):
            print(fn, os.path.getsize(os.path.join(out, fn)))


if __name__ == "__main__":
    main()
