#!/usr/bin/env python3
"""SHA-256 digests of what the bf16 step computes on the smallest shapes at which the forward tile's PROLOGUE (row-id loads,
the W ring prefetch, the X pieces of the first K block, the take verdict in front of the first barrier) can go wrong.  Run on
a build whose outputs are the yardstick (the parent of a change that must stay bit-identical); tests/test_fwd_prologue_gpu.py
holds the printed table as a literal and recomputes it on the build under test.

Digests, inputs and the tie filter are those of scripts/make_step_tail_digests.py (its helpers are imported, the file is not
changed): per case the head weight, exp_avg and exp_avg_sq after 3 AdamW steps, the 3 scalar rows, and the flat gradient of one
grad_step on the first step's batches; every row's top logit is clear of ties.  All cases are bf16, UMLH_MICRO=0, scale 100.

What differs per case is the shape, the environment and how the rows are addressed:
  index "picked"    the rows the tie filter picked from the candidates, as an int64 index vector (the tails script's form)
  index "edges"     the same, but the first and the last row of the table are made clear of ties by construction and stand at
                    the front of every vector, and every other picked row appears twice
  index "identity"  no index vector at all (RowBatch.index = None, single train_step calls): the picked rows are gathered
                    into a compact table on the host, and the step reads rows 0 .. rows-1 of it"""
import hashlib
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tails():
    spec = importlib.util.spec_from_file_location("make_step_tail_digests",
                                                  os.path.join(ROOT, "scripts", "make_step_tail_digests.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _tails()
LR, WD, MARGIN, N_TABLE, ENV_KEYS, FIELDS = T.LR, T.WD, T.MARGIN, T.N_TABLE, T.ENV_KEYS, T.FIELDS
SCALE = 100.0
STANDALONE = {"UMLH_BF16_FUSE": "0"}

# name -> (C, d, image rows, text rows, index form, environment)
CASES = {
    # nks = PD: the prologue ring is the whole W stream of a wave, the slot clamp min(d, nks-1) is live, and the only k-group
    # is the one without refills
    "k128": (1000, 128, 64, 64, "picked", {}),
    "k256": (1000, 256, 64, 64, "picked", {}),                      # one refill group, then the last
    "k512_index_edges": (1000, 512, 96, 40, "edges", {}),          # cfg2's K, one X block: the X address arithmetic
    "k1024_two_blocks": (1000, 1024, 32, 32, "picked", {}),        # the second X block is staged with refills in flight
    # rows clamped to the segment's last row; wave 4 has one live class, waves 5-7 none -- and prefetch all the same
    "partial_dead_waves": (513, 256, 33, 1, "picked", {}),
    "identity_rows": (1000, 256, 64, 64, "identity", {}),
    # the narrow instantiations (CTW, WC) = (1,1), (1,2), (1,4), (1,8), (2,8): several rows per wave-load, XK = 128 / 256 / 512
    "narrow_c32": (32, 256, 40, 24, "picked", {}),
    "narrow_c64": (64, 256, 40, 24, "picked", {}),
    "narrow_c128": (128, 256, 40, 24, "picked", {}),
    "narrow_c256": (256, 256, 40, 24, "picked", {}),
    "narrow_c512": (512, 256, 40, 24, "picked", {}),
    # two sample tiles per wave (stand-alone kernels only): instantiations (2,8,2) and (4,8,2)
    "stw2_c512": (512, 256, 64, 64, "picked", dict(STANDALONE, UMLH_BF16_STW="2")),
    "stw2_c1000": (1000, 256, 64, 64, "picked", dict(STANDALONE, UMLH_BF16_STW="2")),
    # k256 on 3 workgroups / with every fourth workgroup leaving its home tiles to others / through the stand-alone kernels:
    # the cold path, a forward tile that returns at the take verdict with loads in flight, a forward tile taken inside a dW wait
    "grid3": (1000, 256, 64, 64, "picked", {"UMLH_STEP_GRID": "3"}),
    "lazy": (1000, 256, 64, 64, "picked", {"UMLH_STEP_LAZY": "1"}),
    "launch_per_kernel": (1000, 256, 64, 64, "picked", dict(STANDALONE)),
}
# the environment variants and identity_rows run k256's inputs
_K256 = ("k256", "identity_rows", "grid3", "lazy", "launch_per_kernel")
SEEDS = {name: (102 if name in _K256 else 101 + k) for k, name in enumerate(CASES)}


def inputs(name):
    """Host inputs of a case: table rows and labels of both modalities, the initial weight, per-step candidate row ids."""
    C, d, ri, rt, form, _ = CASES[name]
    rng = np.random.default_rng(SEEDS[name])
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    w = unit(rng.standard_normal((C, d)))
    tabs = []
    for m in range(2):
        x = unit(rng.standard_normal((N_TABLE, d)))
        y = rng.integers(0, C, N_TABLE)
        y[: min(C, N_TABLE) // 2] = np.arange(C - min(C, N_TABLE) // 2, C)      # the last classes (the padded tile's) are somebody's label
        if form == "edges":
            # the table's first and last row lean on one class row each: their top logit (about 0.9) is clear of every other
            # (a few 0.1 at the most) by far more than MARGIN, whatever three steps at LR do to the weights
            for r, c in ((0, 7 + m), (N_TABLE - 1, C - 3 - m)):
                x[r] = unit((w[c] + 0.4 * x[r])[None])[0]
        tabs.append((x, y.astype(np.int64)))
    ids = [[rng.integers(0, N_TABLE, 8 * r + 8) for r in (ri, rt)] for _ in range(3)]   # candidates: the tie filter picks r of them
    return w, tabs, ids


def _rows(name, cand, ok, r, what):
    """The r row ids of one modality for one step."""
    if CASES[name][4] != "edges":
        return T._pick(cand, ok, r, what)
    edges = np.array([0, N_TABLE - 1], dtype=np.int64)
    if not ok[edges].all():
        raise RuntimeError(f"{what}: the table's first or last row is not clear of ties")
    body = T._pick(cand, ok, (r - 2 + 1) // 2, what)
    return np.ascontiguousarray(np.concatenate([edges, np.repeat(body, 2)])[:r], dtype=np.int64)


def run_case(name, setenv=None, delenv=None, device="cuda:0"):
    """{field: sha256 hex} of a case on the library that is loaded.  setenv / delenv: pytest's monkeypatch methods (the
    variables are read when an engine is created); by default os.environ is changed and put back."""
    pkg = os.path.join(ROOT, "unpaired-multimodal-learning_amd")
    if pkg not in sys.path:
        sys.path.insert(0, pkg)
    import torch
    import umlh
    C, d, ri, rt, form, env = CASES[name]
    saved = {k: os.environ.get(k) for k in ENV_KEYS}
    setenv = setenv or os.environ.__setitem__
    delenv = delenv or (lambda k: os.environ.pop(k, None))
    for k in ENV_KEYS:
        delenv(k)
    setenv("UMLH_MICRO", "0")      # steps of at most four 16-row tiles would otherwise run as the micro step, which has no forward tile
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
            e = umlh.HeadEngine(d, d, C, optimizer="adamw", weight_decay=WD, max_rows_img=128, max_rows_txt=128,
                                precision="bf16", device=device)
            e.w_head.copy_(dev(w))
            e.scales.fill_(SCALE)
            return e

        def clear_rows(weight, step):
            return [_rows(name, cand[step][m], T._gaps(tabs[m][0], weight) >= MARGIN, r, f"{name} step {step} modality {m}")
                    for m, r in enumerate((ri, rt))]

        def batch(m, rows):
            if form != "identity":
                return umlh.RowBatch(tables[m][0], tables[m][1], dev(rows), feats_bf16=tables[m][2])
            f = dev(tabs[m][0][rows])                        # a compact table: the step reads its rows 0 .. rows-1
            return umlh.RowBatch(f, dev(tabs[m][1][rows]), None, feats_bf16=umlh.to_bf16(f))

        e = engine()
        scal = torch.zeros(3, umlh.N_SCALARS, device=device)
        first = None
        for s in range(3):                                   # one call per step: the tie filter sees the weights it runs on
            rows = clear_rows(e.w_head.cpu().numpy(), s)
            first = first or rows
            if form == "identity":
                e.train_step(batch(0, rows[0]), batch(1, rows[1]), LR, s + 1, scalars_out=scal[s])
            else:
                e.train_steps(tables[0], [dev(rows[0])], tables[1], [dev(rows[1])], [LR], s + 1, scalars_out=scal[s:s + 1])
            torch.cuda.synchronize()
        assert e.step_status() == (0, 0, 0, 0)
        launches = e.step_launches()
        assert (launches > 0) == (env.get("UMLH_BF16_FUSE") != "0"), launches
        out = {"w_head": e.w_head, "exp_avg": e.m_head, "exp_avg_sq": e.v_head, "scalars": scal}
        g = engine()
        # (as in the tails script: the digest covers the C x d head gradient; the scale is fixed in every case)
        out["grad"] = g.grad_step(batch(0, first[0]), batch(1, first[1]))[: C * d]
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
    print(f"# digests of scripts/make_fwd_prologue_digests.py, tree at commit {rev}")
    print("DIGESTS = {")
    for name in CASES:
        r = run_case(name)
        print(f'    "{name}": {{')
        for k in FIELDS:
            print(f'        "{k}": "{r[k]}",')
        print("    },")
    print("}", flush=True)


if __name__ == "__main__":
    main()
