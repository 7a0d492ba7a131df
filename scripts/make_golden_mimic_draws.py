"""Records ``multibench.mimic.draw_mimic_noise(7, levels=3, rng=11)``: tests/golden/mimic_draws.npz, replayed by
tests/test_robust_cpu.py.  The file pins the order of the host draws of the MIMIC noise levels, call for call.

    python scripts/make_golden_mimic_draws.py [--package path/to/unpaired-multimodal-learning_amd]

Run it against the package of the commit whose draws are to be kept (``--package``: that commit's checkout), never against the
code the test is about to check.  The committed file was recorded from the last commit in which ``draw_mimic_noise`` called
the public ``draw_timeseries_noise`` twice per level, before the draw function was split into a resolving and an inner part.
Pure numpy: no GPU, no library."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("drop", "carry", "eps", "elem", "keep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--package", default=os.path.join(ROOT, "unpaired-multimodal-learning_amd"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "mimic_draws.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    from multibench.mimic import draw_mimic_noise
    drawn = draw_mimic_noise(7, levels=3, rng=11)
    np.savez_compressed(args.out, **{f"{k}/{key}": lv[key] for k, lv in enumerate(drawn) for key in KEYS})
    print(f"{args.out}: {os.path.getsize(args.out)} bytes, {len(drawn)} levels")


if __name__ == "__main__":
    main()
