#!/usr/bin/env python3
"""SHA-256 digests of what the fp32 (parity mode) step and the fp32 GEMM entry point compute, on the smallest shapes that reach
every instantiation of the kernels of csrc/umlh_kernels_f32.hip.  Run on a build whose outputs are the yardstick (the parent of a
change that must stay bit-identical): it writes tests/golden/f32_path_digests.json, which tests/test_f32_digests_gpu.py and
tests/test_gemm_f32_gpu.py compare, as strings, with the same digests of the build under test.

Step cases go through HeadEngine.train_step / grad_step (the general path; train_steps may take the micro kernel).  Per case:
head weight, exp_avg and exp_avg_sq after 3 AdamW steps, the 3 scalar rows, and the flat gradient of one grad_step on the first
step's batches (fresh engine); the projected head adds its projection weight.  Inputs come from numpy.random.default_rng on the
host and are uploaded.

  fwd_ce_f32<CTW, WC, MODE>   C = 20, 64, 100, 200, 513, 1000 are the six (CTW, WC) pairs (1,1) (1,2) (1,4) (1,8) (2,8) (4,8);
                              d = 40 is MODE 0 (guarded loads), d = 48 MODE 1 (K % 16 == 0, K % 32 != 0), d = 96 MODE 3 and,
                              under UMLH_F32_X3=0, MODE 2.  At C = 20 (256-row block, X block of 64 columns) d = 96 is two X
                              blocks, the second one short; C = 1000, d = 544 is two X blocks at 32 rows per block.
  dw_f32x3 / dw_f32           C = 1000, d = 544: M N = 544 000 >= 8 * 128 * 128
  gemm_f32<0,1,*>             the dW GEMM of every other case
  gemm_f32<0,0,*>, <1,1,*>    the projected head (d_img 72, d 96, C 100): gathered rows, dH^T = W^T dZ^T
  learnable scale, a step without text rows: one case each
Rows are ragged (33 + 1, 70 + 31): rows past the segment and a class tile that straddles C are both present.

The switches are read once per process, so every environment (the default and UMLH_F32_X3=0 for the step cases; the four of
tests/_gemm_ref.py: ENVS for the GEMM table) runs in a fresh child, one after another.  Every child runs twice before the table
is written, and a disagreement between the two runs refuses it: the yardstick must be deterministic before it is recorded."""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unpaired-multimodal-learning_amd")
TESTS = os.path.join(ROOT, "tests")
TABLE = os.path.join(TESTS, "golden", "f32_path_digests.json")
LR, WD, SCALE, N_TABLE = 1e-3, 0.01, 100.0, 256
SWITCHES = ("UMLH_F32_FWD", "UMLH_F32_X3", "UMLH_F32_TM", "UMLH_F32_DW")
STEP_ENVS = {"default": {}, "x3_off": {"UMLH_F32_X3": "0"}}
_ROWS = ((33, 1), (70, 31))


def _case(C, d, rows, d_img=None, learn=False, no_text_step=None):
    return dict(C=C, d=d, d_img=d_img, rows=rows, learn=learn, no_text_step=no_text_step)


STEP_CASES = {f"c{C}_d{d}": _case(C, d, _ROWS[(i + j) % 2])
              for i, C in enumerate((20, 64, 100, 200, 513, 1000)) for j, d in enumerate((40, 48, 96))}
STEP_CASES.update({
    "c1000_d544": _case(1000, 544, (70, 31)),
    "proj_c100_d72_d96": _case(100, 96, (70, 31), d_img=72),
    "learnable_scale_c100_d96": _case(100, 96, (33, 1), learn=True),
    "no_text_step_c200_d48": _case(200, 48, (70, 31), no_text_step=1),
})


def inputs(name):
    """Host inputs of a step case: initial head weight, projection weight or None, (rows, labels) tables of both modalities,
    row ids per step."""
    c = STEP_CASES[name]
    rng = np.random.default_rng(1 + list(STEP_CASES).index(name))
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    w = unit(rng.standard_normal((c["C"], c["d"])))
    wp = (rng.standard_normal((c["d"], c["d_img"])) / np.sqrt(c["d_img"])).astype(np.float32) if c["d_img"] else None
    tabs = []
    for width in (c["d_img"] or c["d"], c["d"]):
        x = unit(rng.standard_normal((N_TABLE, width)))
        y = rng.integers(0, c["C"], N_TABLE)
        y[:2] = (c["C"] - 1, 0)                                   # the last class (the padded tile's) is somebody's label
        tabs.append((x, y.astype(np.int64)))
    ids = [[rng.integers(0, N_TABLE, r).astype(np.int64) for r in c["rows"]] for _ in range(3)]
    for s in range(3):
        ids[s][0][0] = 0                                          # (table row 0 carries the last class)
    return w, wp, tabs, ids


def run_case(name, device="cuda:0"):
    """{field: sha256 hex} of a step case on the library that is loaded, under the switches of this process."""
    import torch
    import umlh
    c = STEP_CASES[name]
    C, d, d_img = c["C"], c["d"], c["d_img"] or c["d"]
    w, wp, tabs, ids = inputs(name)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    tables = [(dev(x), dev(y)) for x, y in tabs]

    def engine():
        e = umlh.HeadEngine(d_img, d, C, has_proj=wp is not None, optimizer="adamw", weight_decay=WD, learnable_temp=c["learn"],
                            max_rows_img=128, max_rows_txt=128, precision="fp32", device=device)
        e.w_head.copy_(dev(w))
        if wp is not None:
            e.w_proj.copy_(dev(wp))
        e.scales.fill_(SCALE)
        return e

    batch = lambda m, s: umlh.RowBatch(tables[m][0], tables[m][1], dev(ids[s][m]))
    e = engine()
    scal = torch.zeros(3, umlh.N_SCALARS, device=device)
    for s in range(3):
        e.train_step(batch(0, s), None if c["no_text_step"] == s else batch(1, s), lr=LR, step=s + 1, scalars_out=scal[s])
        torch.cuda.synchronize()
    out = {"w_head": e.w_head, "exp_avg": e.m_head, "exp_avg_sq": e.v_head, "scalars": scal}
    if wp is not None:
        out["w_proj"] = e.w_proj
    g = engine()
    # (the message behind the parameter gradients -- scale gradients of a fixed scale -- is not all written by every step)
    n_grad = C * d + (d * d_img if wp is not None else 0) + (2 if c["learn"] else 0)
    out["grad"] = g.grad_step(batch(0, 0), batch(1, 0))[:n_grad]
    torch.cuda.synchronize()
    res = {}
    for k, t in out.items():
        a = t.detach().cpu().contiguous().numpy()
        assert np.isfinite(a).all(), (name, k)
        res[k] = hashlib.sha256(a.tobytes()).hexdigest()
    return res


def _child_env(over):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(over)
    return env


def step_digests(env_name):
    """{case: {field: digest}} of every step case, computed in a fresh child process under STEP_ENVS[env_name]."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step-child"], env=_child_env(STEP_ENVS[env_name]),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (env_name, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("F32_STEP_DIGESTS ")]
    assert len(line) == 1, r.stdout[-1000:]
    return json.loads(line[0].split(" ", 1)[1])


def gemm_digests():
    """{case id: {environment: digest}} of the [M, N] windows of the GEMM table, by the children of tests/test_gemm_f32_gpu.py."""
    if TESTS not in sys.path:
        sys.path.insert(0, TESTS)
    import pathlib
    import test_gemm_f32_gpu as T
    with tempfile.TemporaryDirectory() as tmp:
        return T.window_digests(T._run_children(pathlib.Path(tmp)))


def load_table():
    with open(TABLE) as f:
        return json.load(f)


def main():
    if sys.argv[1:] == ["--step-child"]:
        sys.path[:0] = [ROOT, PKG]
        print("F32_STEP_DIGESTS " + json.dumps({name: run_case(name) for name in STEP_CASES}))
        return
    runs = []
    for _ in range(2):
        runs.append({"step": {name: step_digests(name) for name in STEP_ENVS}, "gemm": gemm_digests()})
    if runs[0] != runs[1]:
        diff = [(part, k) for part in ("step", "gemm") for k in runs[0][part] if runs[0][part][k] != runs[1][part].get(k)]
        sys.exit(f"two runs of the same build disagree, nothing written: {diff}")
    # usage: make_f32_digests.py [output file [commit label]]   (the label for trees without their git history)
    rev = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"],
                                                               capture_output=True, text=True).stdout.strip()
    out = sys.argv[1] if len(sys.argv) > 1 else TABLE
    with open(out, "w") as f:
        json.dump({"recorded_from": rev or "unknown", **runs[0]}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {out}: {len(STEP_CASES)} step cases x {len(STEP_ENVS)} environments, {len(runs[0]['gemm'])} GEMM cases")


if __name__ == "__main__":
    main()
