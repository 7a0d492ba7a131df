"""Time of the outlier-clamp kernels (umlh.align.row_abs_quantile / abs_kth / the clamp, alone through the C ABI with
preallocated buffers), of whole remove_outliers / prepare_features calls, and of the torch-op form of the same quantities on
the same GPU: ``abs`` + ``quantile(dim=1)`` + ``mean`` + ``clamp`` (+ ``F.normalize``), and ``abs().view(-1).sort()`` for
``exact``.  torch.quantile refuses inputs above 16 777 216 elements; there the torch form takes the same two order statistics
from ``abs().sort(dim=1)`` (what quantile does inside) and the line says so.

    python scripts/bench_outliers.py [--reps R] [--out profiles/outliers_bench.txt]

Device time between two events, (median, min, max) over R calls after two warm-up calls.  Beside each HIP kernel: the bytes it
must move (selection: one read of the matrix; clamp: one read and one write) and the rate that gives."""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (HERE, os.path.join(HERE, "unpaired-multimodal-learning_amd"), os.path.join(HERE, "scripts")):
    sys.path.insert(0, p)

DEV = "cuda:0"
SHAPES = ((50_000, 512), (1000, 1024), (64, 8192), (1000, 15_000), (50_000, 300))
Q = 0.95


def torch_bound(x, q):
    """(q_val, how) of the reference's non-exact branch (metrics.py:336) in torch ops."""
    import torch
    a = x.abs().flatten(start_dim=1)
    if a.numel() <= 16_777_216:
        return torch.quantile(a, q, dim=1).mean(), "quantile"
    s = a.sort(dim=1).values
    pos = q * (a.shape[1] - 1)
    lo = int(pos)
    hi = min(lo + 1, a.shape[1] - 1)
    return torch.lerp(s[:, lo], s[:, hi], pos - lo).mean(), "sort(dim=1) (quantile refuses > 2^24 elements)"


def main(args):
    import torch
    import torch.nn.functional as F
    import umlh
    from umlh import _glue as glue
    from umlh._lib import check, load_library
    from bench_knn import timed
    A, lib = umlh.align, load_library()
    lines = [json.dumps({"device": torch.cuda.get_device_name(0), "q": Q, "reps": args.reps,
                         "times": "device us between events: [median, min, max]"})]

    def say(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    def t(fn):
        return [round(v, 1) for v in timed(fn, args.reps, warm=2)]

    def rate(nbytes, us):
        return round(nbytes / (us[0] * 1e-6) / 1e12, 3)

    for n, d in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(n + d)
        x = torch.randn(n, d, device=DEV, generator=g)
        shape = f"{n} x {d}"
        nbytes = n * d * 4
        st = glue.stream(x.device)
        quant, q_val = torch.empty(n, device=DEV), torch.empty((), device=DEV)
        s_q, b_q = glue.scratch("umlh_outlier_scratch_bytes", x.device, kind=A.KIND_ROW_QUANTILE, n=n, d=d)
        s_k, b_k = glue.scratch("umlh_outlier_scratch_bytes", x.device, kind=A.KIND_ABS_KTH, n=n, d=d)
        out = torch.empty_like(x)
        k = int(Q * x.numel())
        sel = lambda: check(lib.umlh_row_abs_quantile(x.data_ptr(), n, d, d, Q, None, None, quant.data_ptr(), None, q_val.data_ptr(),
                                                      s_q.data_ptr(), b_q, st), "row")
        kth = lambda: check(lib.umlh_abs_kth(x.data_ptr(), n, d, d, k, q_val.data_ptr(), s_k.data_ptr(), b_k, st), "kth")
        clamp = lambda nrm: check(lib.umlh_clamp_rows(x.data_ptr(), n, d, d, q_val.data_ptr(), nrm, out.data_ptr(), d, st), "clamp")
        path = "wave per row" if d <= A.ROW_QUANTILE_WAVE_COLS else "row in LDS" if d <= A.ROW_QUANTILE_LDS_COLS else "streamed"
        us = t(sel)
        say({"what": "umlh_row_abs_quantile alone (select + mean, 3 launches)", "shape": shape, "path": path, "us": us,
             "bytes_it_must_move": nbytes, "TB_per_s": rate(nbytes, us)})
        us = t(kth)
        say({"what": "umlh_abs_kth alone (memset + 4 launches; each pass reads the matrix)", "shape": shape, "us": us,
             "bytes_it_must_move": nbytes, "bytes_it_reads": 4 * nbytes, "TB_per_s_of_must_move": rate(nbytes, us),
             "TB_per_s_of_read": rate(4 * nbytes, us)})
        sel()
        for nrm in (0, 1):
            us = t(lambda: clamp(nrm))
            say({"what": f"umlh_clamp_rows alone, normalize={nrm}", "shape": shape, "path": path if nrm else "elementwise", "us": us,
                 "bytes_it_must_move": 2 * nbytes, "TB_per_s": rate(2 * nbytes, us)})
        ref_q, how = torch_bound(x, Q)
        mine = A.row_abs_quantile(x, Q)[0]
        ref_k = x.view(-1).abs().sort().values[k]
        assert abs(float(mine) - float(ref_q)) <= 1e-5 * float(ref_q) and float(A.abs_kth(x, k)) == float(ref_k)
        assert torch.equal(A.remove_outliers(x, Q, exact=True), x.clamp(-ref_k, ref_k))
        say({"what": "remove_outliers(q), whole call", "shape": shape, "hip_us": t(lambda: A.remove_outliers(x, Q)),
             "torch_us": t(lambda: (lambda b: x.clamp(-b, b))(torch_bound(x, Q)[0])), "torch_form": f"abs + {how} + mean + clamp"})
        say({"what": "remove_outliers(q, exact=True), whole call", "shape": shape,
             "hip_us": t(lambda: A.remove_outliers(x, Q, exact=True)),
             "torch_us": t(lambda: (lambda b: x.clamp(-b, b))(x.view(-1).abs().sort().values[k])),
             "torch_form": "abs().view(-1).sort() + clamp"})
        say({"what": "prepare_features(q), whole call", "shape": shape, "hip_us": t(lambda: A.prepare_features(x, Q)),
             "torch_us": t(lambda: (lambda b: F.normalize(x.clamp(-b, b), dim=-1))(torch_bound(x, Q)[0])),
             "torch_form": f"abs + {how} + mean + clamp + F.normalize"})
        del x, out
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "outliers_bench.txt"))
    main(ap.parse_args())
