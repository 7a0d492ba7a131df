import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "unpaired-multimodal-learning_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden_dir():
    return GOLDEN


class Golden(dict):
    """The arrays of one fixture by name; ``files`` lists the names, as numpy's NpzFile does."""

    @property
    def files(self):
        return list(self)


def load_golden(name):
    """tests/golden/<name>.npz, merged with <name>.part1.npz, <name>.part2.npz, ... when a fixture is stored in parts
    (every committed file stays under 1 MiB)."""
    import numpy as np
    g = Golden()
    paths, k = [os.path.join(GOLDEN, name + ".npz")], 1
    while os.path.exists(os.path.join(GOLDEN, f"{name}.part{k}.npz")):
        paths.append(os.path.join(GOLDEN, f"{name}.part{k}.npz"))
        k += 1
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            for key in z.files:
                assert key not in g, f"{p}: array {key!r} also stored in another part of fixture {name!r}"
                g[key] = z[key]
    return g
