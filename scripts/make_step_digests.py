#!/usr/bin/env python3
"""Record the step's bit checks: SHA-256 digests of what the head step (bf16 and fp32) and the fp32 GEMM entry point compute on
the cases of tests/_step_digests.py.  Run on a build whose outputs are the yardstick (the parent of a change that must stay
bit-identical); tests/test_step_digests_gpu.py and tests/test_gemm_f32_gpu.py compare the tables, as strings, with the same
digests of the build under test.

usage: make_step_digests.py SUITE|all [--out DIR] [--label COMMIT]
  SUITE    step_tails, fwd_prologue (both in bf16_step_digests.json) or f32_step (f32_path_digests.json, with the GEMM table of
           the four environments of tests/_gemm_ref.py: ENVS, computed by the children of tests/test_gemm_f32_gpu.py)
  --out    where the tables are written (default tests/golden; a suite that is not recorded keeps its committed entry)
  --label  "recorded_from" for trees without their git history (default: the short commit)

Every environment of a suite runs in a fresh child, one after another, and every suite is computed twice: a disagreement between
the two runs refuses the table.  The yardstick must be deterministic before it is recorded."""
import argparse
import json
import os
import pathlib
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _step_digests as D


def gemm_digests():
    """{case id: {environment: digest}} of the [M, N] windows of the GEMM table, by the children of tests/test_gemm_f32_gpu.py."""
    import test_gemm_f32_gpu as T
    with tempfile.TemporaryDirectory() as tmp:
        return T.window_digests(T._run_children(pathlib.Path(tmp)))


def compute(suite):
    table = {"step": {name: D.digests_in_child(suite, env) for name, env in D.PROCESS_ENVS[suite].items()}}
    if suite == "f32_step":
        table["gemm"] = gemm_digests()
    return table


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("suite", choices=list(D.SUITES) + ["all"])
    ap.add_argument("--out", default=os.path.dirname(D.BF16_TABLE))
    ap.add_argument("--label")
    a = ap.parse_args()
    rev = a.label or subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                    text=True).stdout.strip() or "unknown"
    with open(D.BF16_TABLE) as f:
        bf16 = json.load(f)
    files = {}
    for suite in (list(D.SUITES) if a.suite == "all" else [a.suite]):
        first, second = compute(suite), compute(suite)
        if first != second:
            diff = [(part, k) for part in first for k in first[part] if first[part][k] != second[part].get(k)]
            sys.exit(f"{suite}: two runs of the same build disagree, nothing written: {diff}")
        if suite == "f32_step":
            files[os.path.basename(D.F32_TABLE)] = {"recorded_from": rev, **first}
        else:
            bf16[suite] = {"recorded_from": rev, "cases": first["step"]["default"]}
            files[os.path.basename(D.BF16_TABLE)] = bf16
        print(f"{suite}: {len(D.SUITES[suite])} cases x {len(D.PROCESS_ENVS[suite])} environments, twice the same")
    os.makedirs(a.out, exist_ok=True)
    for name, table in files.items():
        with open(os.path.join(a.out, name), "w") as f:
            json.dump(table, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", os.path.join(a.out, name))


if __name__ == "__main__":
    main()
