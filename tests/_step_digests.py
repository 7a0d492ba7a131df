"""The recorded bit checks of the head step: cases, host inputs and the one runner that turns a case into SHA-256 digests.

Per case: head weight, exp_avg and exp_avg_sq after 3 AdamW steps, the 3 scalar rows, and the flat gradient of one grad_step on
the first step's batches (fresh engine); the projected head adds its projection weight.  Inputs come from
numpy.random.default_rng on the host and are uploaded: nothing depends on the device RNG.  scripts/make_step_digests.py records
the tables under tests/golden/ on a build whose outputs are the yardstick; tests/test_step_digests_gpu.py (which lists why each
case exists) recomputes them on the build under test, tests/test_step_digests_cpu.py holds tables and inputs to this file.

Ties (bf16 cases).  A step's rows are taken only from table rows whose two largest logits (float64, on the bf16-rounded operands
the kernel multiplies: the rows' bf16 shadow and the bf16 rounding of the weights that step reads, read back before it) lie at
least MARGIN = 0.01 apart -- four orders of magnitude above the fp32 accumulation error of a 512-term dot product of operands
below 1 (512 * 2^-24 = 3e-5 at the very most).  So the top-1 class of every row is the same under any summation order and the hit
counts in the scalar rows are unambiguous.

How the rows of a case are addressed (Case.index):
  "picked"    the rows the tie filter picked from the candidates, as an int64 index vector, through train_steps
  "edges"     the same, but the first and the last row of the table are made clear of ties by construction and stand at the
              front of every vector, and every other picked row appears twice
  "identity"  no index vector at all (RowBatch.index = None, single train_step calls): the picked rows are gathered into a
              compact table on the host, and the step reads rows 0 .. rows-1 of it
  "ids"       the fp32 cases: drawn row ids as they are, no tie filter, single train_step calls (the general path; train_steps
              may take the micro kernel)"""
import hashlib
import json
import os
import subprocess
import sys
import typing

import numpy as np

from _switches import child_env, engine_env

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
PKG = os.path.join(ROOT, "unpaired-multimodal-learning_amd")
BF16_TABLE = os.path.join(TESTS, "golden", "bf16_step_digests.json")
F32_TABLE = os.path.join(TESTS, "golden", "f32_path_digests.json")
LR, WD, MARGIN = 1e-3, 0.01, 0.01
_TAG = "STEP_DIGESTS "


class Case(typing.NamedTuple):
    name: str
    precision: str                  # "bf16" | "fp32"
    C: int
    d: int
    rows: tuple                     # (image rows, text rows) of every step
    seed: int
    d_img: int = 0                  # width of the image rows in front of a projection; 0: no projection
    scale: float = 100.0
    learn: bool = False             # learnable scale
    index: str = "picked"
    no_text_step: int = -1          # the step that runs without text rows
    n_table: int = 512
    env: dict = {}                  # engine-scope switches


_FUSE0 = {"UMLH_BF16_FUSE": "0"}


def _bf16(name, C, d, ri, rt, seed, **kw):
    return Case(name, "bf16", C, d, (ri, rt), seed, **kw)


SUITES = {
    # the environment variants run the first case's inputs
    "step_tails": [
        _bf16("both_halves_c1000", 1000, 128, 64, 64, 1),
        _bf16("wave4_one_class_c513", 513, 128, 33, 1, 2),
        _bf16("upper_half_padding_c512", 512, 128, 32, 32, 3),
        _bf16("wave0_only_c100", 100, 128, 32, 32, 4),
        _bf16("learnable_scale_d512", 1000, 512, 96, 40, 5, learn=True),
        _bf16("negative_scale", 1000, 128, 64, 64, 6, scale=-100.0),
        _bf16("grid3", 1000, 128, 64, 64, 1, env={"UMLH_STEP_GRID": "3"}),
        _bf16("lazy", 1000, 128, 64, 64, 1, env={"UMLH_STEP_LAZY": "1"}),
        _bf16("launch_per_kernel", 1000, 128, 64, 64, 1, env=_FUSE0),
    ],
    # the environment variants and identity_rows run k256's inputs
    "fwd_prologue": [
        _bf16("k128", 1000, 128, 64, 64, 101),
        _bf16("k256", 1000, 256, 64, 64, 102),
        _bf16("k512_index_edges", 1000, 512, 96, 40, 103, index="edges"),
        _bf16("k1024_two_blocks", 1000, 1024, 32, 32, 104),
        _bf16("partial_dead_waves", 513, 256, 33, 1, 105),
        _bf16("identity_rows", 1000, 256, 64, 64, 102, index="identity"),
        _bf16("narrow_c32", 32, 256, 40, 24, 107),
        _bf16("narrow_c64", 64, 256, 40, 24, 108),
        _bf16("narrow_c128", 128, 256, 40, 24, 109),
        _bf16("narrow_c256", 256, 256, 40, 24, 110),
        _bf16("narrow_c512", 512, 256, 40, 24, 111),
        _bf16("stw2_c512", 512, 256, 64, 64, 112, env=dict(_FUSE0, UMLH_BF16_STW="2")),
        _bf16("stw2_c1000", 1000, 256, 64, 64, 113, env=dict(_FUSE0, UMLH_BF16_STW="2")),
        _bf16("grid3", 1000, 256, 64, 64, 102, env={"UMLH_STEP_GRID": "3"}),
        _bf16("lazy", 1000, 256, 64, 64, 102, env={"UMLH_STEP_LAZY": "1"}),
        _bf16("launch_per_kernel", 1000, 256, 64, 64, 102, env=_FUSE0),
    ],
}


def _f32_suite():
    """Rows are ragged (33 + 1, 70 + 31): rows past the segment and a class tile that straddles C are both present."""
    ragged = ((33, 1), (70, 31))
    grid = [(f"c{C}_d{d}", C, d, ragged[(i + j) % 2], {})
            for i, C in enumerate((20, 64, 100, 200, 513, 1000)) for j, d in enumerate((40, 48, 96))]
    extra = [("c1000_d544", 1000, 544, (70, 31), {}),
             ("proj_c100_d72_d96", 100, 96, (70, 31), dict(d_img=72)),
             ("learnable_scale_c100_d96", 100, 96, (33, 1), dict(learn=True)),
             ("no_text_step_c200_d48", 200, 48, (70, 31), dict(no_text_step=1))]
    return [Case(name, "fp32", C, d, rows, 1 + k, index="ids", n_table=256, **kw) for k, (name, C, d, rows, kw) in enumerate(grid + extra)]


SUITES["f32_step"] = _f32_suite()
# switches read once per process: every environment of a suite is one fresh child (digests_in_child)
PROCESS_ENVS = {"step_tails": {"default": {}}, "fwd_prologue": {"default": {}},
                "f32_step": {"default": {}, "x3_off": {"UMLH_F32_X3": "0"}}}


def fields(case):
    return ("w_head", "exp_avg", "exp_avg_sq", "scalars") + (("w_proj",) if case.d_img else ()) + ("grad",)


def inputs(case):
    """Host inputs of a case, in the order of the generator's draws: initial head weight, projection weight or None, (rows,
    labels) tables of both modalities, per step the row ids (fp32) or the candidates the tie filter picks from (bf16)."""
    c, n = case, case.n_table
    bf16 = c.precision == "bf16"
    rng = np.random.default_rng(c.seed)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)
    w = unit(rng.standard_normal((c.C, c.d)))
    wp = (rng.standard_normal((c.d, c.d_img)) / np.sqrt(c.d_img)).astype(np.float32) if c.d_img else None
    tabs = []
    for m, width in enumerate((c.d_img or c.d, c.d)):
        x = unit(rng.standard_normal((n, width)))
        y = rng.integers(0, c.C, n)
        if bf16:
            y[: min(c.C, n) // 2] = np.arange(c.C - min(c.C, n) // 2, c.C)     # the last classes (the padded tile's) are somebody's label
        else:
            y[:2] = (c.C - 1, 0)                                               # the last class (the padded tile's) is somebody's label
        if c.index == "edges":
            # the table's first and last row lean on one class row each: their top logit (about 0.9) is clear of every other
            # (a few 0.1 at the most) by far more than MARGIN, whatever three steps at LR do to the weights
            for r, k in ((0, 7 + m), (n - 1, c.C - 3 - m)):
                x[r] = unit((w[k] + 0.4 * x[r])[None])[0]
        tabs.append((x, y.astype(np.int64)))
    if bf16:
        ids = [[rng.integers(0, n, 8 * r + 8) for r in c.rows] for _ in range(3)]     # candidates: the tie filter picks r of them
    else:
        ids = [[rng.integers(0, n, r).astype(np.int64) for r in c.rows] for _ in range(3)]
        for s in range(3):
            ids[s][0][0] = 0                                                   # (table row 0 carries the last class)
    return w, wp, tabs, ids


def inputs_digest(case):
    """SHA-256 over the bytes of inputs(case), array after array (tests/golden/step_digest_inputs.json)."""
    w, wp, tabs, ids = inputs(case)
    h = hashlib.sha256()
    for a in [w] + ([wp] if wp is not None else []) + [a for tab in tabs for a in tab] + [a for step in ids for a in step]:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _bf16_round(a):
    """Round-to-nearest-even to bf16, as float64 (what the kernel's operands hold)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def _gaps(x, w):
    z = _bf16_round(x) @ _bf16_round(w).T
    z.sort(axis=1)
    return z[:, -1] - z[:, -2]


def _pick(cand, ok, r, what):
    keep = cand[ok[cand]][:r]
    if len(keep) < r:
        raise RuntimeError(f"{what}: fewer than {r} candidate rows clear of ties; change the seed")
    return np.ascontiguousarray(keep, dtype=np.int64)


def _rows(case, cand, ok, r, what):
    """The r row ids of one modality for one step of a bf16 case."""
    if case.index != "edges":
        return _pick(cand, ok, r, what)
    edges = np.array([0, case.n_table - 1], dtype=np.int64)
    if not ok[edges].all():
        raise RuntimeError(f"{what}: the table's first or last row is not clear of ties")
    body = _pick(cand, ok, (r - 2 + 1) // 2, what)
    return np.ascontiguousarray(np.concatenate([edges, np.repeat(body, 2)])[:r], dtype=np.int64)


def run_case(case, setenv=None, delenv=None, device="cuda:0"):
    """{field: sha256 hex} of a case on the library that is loaded, under the process-scope switches of this process.
    setenv / delenv: pytest's monkeypatch methods, as for engine_env; by default os.environ is changed and put back."""
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    import umlh
    c, bf16 = case, case.precision == "bf16"
    # bf16: steps of at most four 16-row tiles would otherwise run as the micro step, which has none of the tiles under test
    restore = engine_env(setenv, delenv, dict({"UMLH_MICRO": "0"} if bf16 else {}, **c.env))
    try:
        w, wp, tabs, ids = inputs(c)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        tables = []
        for x, y in tabs:
            f = dev(x)
            tables.append((f, dev(y), umlh.to_bf16(f) if bf16 else None))

        def engine():
            e = umlh.HeadEngine(c.d_img or c.d, c.d, c.C, has_proj=wp is not None, optimizer="adamw", weight_decay=WD,
                                learnable_temp=c.learn, max_rows_img=128, max_rows_txt=128, precision=c.precision, device=device)
            e.w_head.copy_(dev(w))
            if wp is not None:
                e.w_proj.copy_(dev(wp))
            e.scales.fill_(c.scale)
            return e

        def clear_rows(weight, step):
            return [_rows(c, ids[step][m], _gaps(tabs[m][0], weight) >= MARGIN, r, f"{c.name} step {step} modality {m}")
                    for m, r in enumerate(c.rows)]

        def batch(m, rows):
            if c.index != "identity":
                return umlh.RowBatch(tables[m][0], tables[m][1], dev(rows), feats_bf16=tables[m][2])
            f = dev(tabs[m][0][rows])                        # a compact table: the step reads its rows 0 .. rows-1
            return umlh.RowBatch(f, dev(tabs[m][1][rows]), None, feats_bf16=umlh.to_bf16(f))

        e = engine()
        scal = torch.zeros(3, umlh.N_SCALARS, device=device)
        first = None
        for s in range(3):                                   # one call per step: the tie filter sees the weights it runs on
            rows = clear_rows(e.w_head.cpu().numpy(), s) if bf16 else ids[s]
            first = first or rows
            if c.index in ("picked", "edges"):
                e.train_steps(tables[0], [dev(rows[0])], tables[1], [dev(rows[1])], [LR], s + 1, scalars_out=scal[s:s + 1])
            else:
                e.train_step(batch(0, rows[0]), None if c.no_text_step == s else batch(1, rows[1]), lr=LR, step=s + 1,
                             scalars_out=scal[s])
            torch.cuda.synchronize()
        if bf16:
            assert e.step_status() == (0, 0, 0, 0)
            launches = e.step_launches()
            assert (launches > 0) == (c.env.get("UMLH_BF16_FUSE") != "0"), launches
        out = {"w_head": e.w_head, "exp_avg": e.m_head, "exp_avg_sq": e.v_head, "scalars": scal}
        if wp is not None:
            out["w_proj"] = e.w_proj
        g = engine()
        # (the message behind the parameter gradients -- scale gradients of a fixed scale, diagnostics that are off -- is not all
        # written by every step: the digest covers the head gradient, the projection's, and the two scale gradients where learnt)
        n_grad = c.C * c.d + c.d * c.d_img + (2 if c.learn else 0)
        out["grad"] = g.grad_step(batch(0, first[0]), batch(1, first[1]))[:n_grad]
        torch.cuda.synchronize()
        if bf16:
            assert g.step_status() == (0, 0, 0, 0)
        res = {}
        for k in fields(c):
            a = out[k].detach().cpu().contiguous().numpy()
            assert np.isfinite(a).all(), (c.name, k)
            res[k] = hashlib.sha256(a.tobytes()).hexdigest()
        return res
    finally:
        restore()


def digests_in_child(suite, process_env):
    """{case: {field: digest}} of every case of a suite, computed in a fresh child process under the switches `process_env`."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", suite], env=child_env(process_env),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (suite, process_env, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith(_TAG)]
    assert len(line) == 1, r.stdout[-1000:]
    return json.loads(line[0][len(_TAG):])


def load_table(suite):
    """{process environment: {case: {field: digest}}} of a suite, as committed."""
    with open(F32_TABLE if suite == "f32_step" else BF16_TABLE) as f:
        table = json.load(f)
    return table["step"] if suite == "f32_step" else {"default": table[suite]["cases"]}


if __name__ == "__main__":
    assert sys.argv[1] == "--child", sys.argv
    sys.path[:0] = [ROOT, PKG]
    print(_TAG + json.dumps({c.name: run_case(c) for c in SUITES[sys.argv[2]]}))
