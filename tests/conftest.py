import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    import torch
    # (device_count() does not initialise the GPU; is_available() does, and tests/test_gpu_dist.py has to start its rank
    # processes from a parent that has not touched the device yet — which is also why that module is moved to the front)
    #
    # Order of the GPU suite (the driver runs `pytest -m gpu -x`): parity evidence first, self-consistency last, so that one
    # property test at a noise floor can never hide an oracle / golden / operator check.
    #   0  test_gpu_dist        (must start its rank processes before this process touches the device)
    #   1  test_gpu_ops         operator level: every kernel against the oracle / torch fp32
    #   2  model tests that compare with the reference's golden vectors or the oracle ("golden" / "oracle" in the name)
    #   3  test_gpu_prune_flow  the reference's own prune test flow
    #   4  everything else      properties at bench size, executor-vs-executor and rerun / layout self-consistency
    def tier(it):
        nid = it.nodeid
        if "test_gpu_dist" in nid:
            return 0
        if "test_gpu_ops" in nid:
            return 1
        if "test_gpu_model" in nid:
            name = nid.split("::", 1)[-1]
            return 2 if ("golden" in name or "oracle" in name) else 4
        if "test_gpu_prune_flow" in nid:
            return 3
        return 1          # CPU modules: unaffected by -m gpu
    items.sort(key=tier)
    if torch.cuda.device_count() > 0:
        return
    skip = pytest.mark.skip(reason="no GPU visible")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        # a fixture above 1 MiB is stored as <name>.npz + <name>.part2.npz ... (tests/golden/common.py: save_golden)
        if name not in cache:
            stem = os.path.join(GOLDEN_DIR, name)
            parts = sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(p[len(stem) + 5:-4]))
            cache[name] = {}
            for p in [stem + ".npz"] + parts:
                cache[name].update(np.load(p, allow_pickle=False))
        return cache[name]

    return load
