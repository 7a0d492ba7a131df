#!/usr/bin/env python3
"""SHA-256 digests of what the bf16 step computes on the smallest shapes at which a tile's tail (everything after its last
MFMA: softmax passes, dZ^T staging and stores, slab epilogue, publish) can go wrong.  Run on a build whose outputs are the
yardstick (the parent of a change that must stay bit-identical); tests/test_step_tails_gpu.py holds the printed table as a
literal and recomputes it on the build under test.

Per case: head weight, exp_avg and exp_avg_sq after 3 AdamW steps (HeadEngine.train_steps), the 3 scalar rows, and the flat
gradient of one grad_step on the first step's batches (fresh engine).  Inputs come from numpy.random.default_rng on the
host and are uploaded: nothing depends on the device RNG.

Ties.  A step's rows are taken only from table rows whose two largest logits (float64, on the bf16-rounded operands the
kernel multiplies: the rows' bf16 shadow and the bf16 rounding of the weights that step reads, read back before it) lie at
least MARGIN = 0.01 apart -- four orders of magnitude above the fp32 accumulation error of a 512-term dot product of
operands below 1 (512 * 2^-24 = 3e-5 at the very most).  So the top-1 class of every row is the same under any summation
order and the hit counts in the scalar rows are unambiguous."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, WD, MARGIN, N_TABLE = 1e-3, 0.01, 0.01, 512
ENV_KEYS = ("UMLH_STEP_GRID", "UMLH_STEP_LAZY", "UMLH_BF16_FUSE", "UMLH_FORCE_DP", "UMLH_BF16_FWD2D", "UMLH_WT", "UMLH_MICRO",
            "UMLH_BF16_STW", "UMLH_DBG_FWD", "UMLH_DBG_DW", "UMLH_DBG_STEP")

# name -> (C, d, image rows, text rows, scale, learnable scale, environment)
CASES = {
    "both_halves_c1000": (1000, 128, 64, 64, 100.0, False, {}),
    "wave4_one_class_c513": (513, 128, 33, 1, 100.0, False, {}),
    "upper_half_padding_c512": (512, 128, 32, 32, 100.0, False, {}),
    "wave0_only_c100": (100, 128, 32, 32, 100.0, False, {}),
    "learnable_scale_d512": (1000, 512, 96, 40, 100.0, True, {}),
    "negative_scale": (1000, 128, 64, 64, -100.0, False, {}),
    "grid3": (1000, 128, 64, 64, 100.0, False, {"UMLH_STEP_GRID": "3"}),
    "lazy": (1000, 128, 64, 64, 100.0, False, {"UMLH_STEP_LAZY": "1"}),
    "launch_per_kernel": (1000, 128, 64, 64, 100.0, False, {"UMLH_BF16_FUSE": "0"}),
}
# the environment variants run the first case's inputs
SEEDS = {name: (1 if name in ("grid3", "lazy", "launch_per_kernel") else 1 + k) for k, name in enumerate(CASES)}
FIELDS = ("w_head", "exp_avg", "exp_avg_sq", "scalars", "grad")


def _bf16(a):
    """Round-to-nearest-even to bf16, as float64 (what the kernel's operands hold)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _gaps(x, w):
    z = _bf16(x) @ _bf16(w).T
    z.sort(axis=1)
    return z[:, -1] - z[:, -2]


def inputs(name):
    """Host inputs of a case: table rows and labels of both modalities, the initial weight, per-step row ids."""
    C, d, ri, rt, scale, learn, _ = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    w = unit(rng.standard_normal((C, d)))
    tabs = []
    for _ in range(2):
        x = unit(rng.standard_normal((N_TABLE, d)))
        y = rng.integers(0, C, N_TABLE)
        y[: min(C, N_TABLE) // 2] = np.arange(C - min(C, N_TABLE) // 2, C)      # the last classes (the padded tile's) are somebody's label
        tabs.append((x, y.astype(np.int64)))
    ids = [[rng.integers(0, N_TABLE, 8 * r + 8) for r in (ri, rt)] for _ in range(3)]   # candidates: the tie filter picks r of them
    return w, tabs, ids


def _pick(cand, ok, r, what):
    keep = cand[ok[cand]][:r]
    if len(keep) < r:
        raise RuntimeError(f"{what}: fewer than {r} candidate rows clear of ties; change the seed")
    return np.ascontiguousarray(keep, dtype=np.int64)


def run_case(name, setenv=None, delenv=None, device="cuda:0"):
    """{field: sha256 hex} of a case on the library that is loaded.  setenv / delenv: pytest's monkeypatch methods (the
    variables are read when an engine is created); by default os.environ is changed and put back."""
    pkg = os.path.join(ROOT, "unpaired-multimodal-learning_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import torch
    import umlh
    C, d, ri, rt, scale, learn, env = CASES[name]
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in ENV_KEYS:
        delenv(k)
    setenv("UMLH_MICRO", "0")      # steps of at most four 16-row tiles would otherwise run as the micro step, which has none of these tails
    for k, v in env.items():
        setenv(k, v)
    try:
        w, tabs, cand = inputs(name)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        tables = []
        for x, y in tabs:
            f = dev(x)
            tables.append((f, dev(y), umlh.to_bf16(f)))

        def engine():
            e = umlh.HeadEngine(d, d, C, optimizer="adamw", weight_decay=WD, learnable_temp=learn, max_rows_img=128,
                                max_rows_txt=128, precision="bf16", device=device)
            e.w_head.copy_(dev(w))
            e.scales.fill_(scale)
            return e

        def clear_rows(weight, step):
            return [_pick(cand[step][m], _gaps(tabs[m][0], weight) >= MARGIN, r, f"{name} step {step} modality {m}")
                    for m, r in enumerate((ri, rt))]

        e = engine()
        scal = torch.zeros(3, umlh.N_SCALARS, device=device)
        first = None
        for s in range(3):                                   # one train_steps call per step: the tie filter sees the weights it runs on
            rows = clear_rows(e.w_head.cpu().numpy(), s)
            first = first or rows
            e.train_steps(tables[0], [dev(rows[0])], tables[1], [dev(rows[1])], [LR], s + 1, scalars_out=scal[s:s + 1])
            torch.cuda.synchronize()
        assert e.step_status() == (0, 0, 0, 0)
        launches = e.step_launches()
        assert (launches > 0) == (env.get("UMLH_BF16_FUSE") != "0"), launches
        out = {"w_head": e.w_head, "exp_avg": e.m_head, "exp_avg_sq": e.v_head, "scalars": scal}
        g = engine()
        batch = lambda m: umlh.RowBatch(tables[m][0], tables[m][1], dev(first[m]), feats_bf16=tables[m][2])
        # (the message behind the head gradient -- scale gradients of a fixed scale, diagnostics that are off -- is not all
        # written by every step: the digest covers the C x d head gradient, and the two scale gradients where they are learnt)
        out["grad"] = g.grad_step(batch(0), batch(1))[: C * d + (2 if learn else 0)]
        torch.cuda.synchronize()
        assert g.step_status() == (0, 0, 0, 0)
        res = {}
        for k in FIELDS:
            a = out[k].detach().cpu().contiguous().numpy()
            assert np.isfinite(a).all(), (name, k)
            res[k] = hashlib.sha256(a.tobytes()).hexdigest()
        return res
    finally:
        for k, v in saved.items():
            if v is None:
                delenv(k)
            else:
                setenv(k, v)


def main():
    import subprocess
    try:
        rev = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        rev = "unknown"
    print(f"# digests of scripts/make_step_tail_digests.py, tree at commit {rev}")
    print("DIGESTS = {")
    for name in CASES:
        r = run_case(name)
        print(f'    "{name}": {{')
        for k in FIELDS:
            print(f'        "{k}": "{r[k]}",')
        print("    },")
    print("}")


if __name__ == "__main__":
    main()
