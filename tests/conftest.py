import os
import sys

# The suite's CPU arithmetic (the oracle, held to tests/golden/ bit for bit in places) is pinned to kernels that round the
# same on Intel and AMD x86-64 CPUs with AVX-512: ATen's AVX-512 kernels, oneDNN capped at its base AVX-512 kernels (no
# AMX / AVX-512 FP16 variants, which only some CPUs have), MKL's conditional-numerical-reproducibility COMPATIBLE branch
# (its other branches differ between vendors in exp()), on a fixed number of threads.  The defaults pick kernels by CPU
# model and thread count, and exp() and the convolutions then differ in the last bits.  tools/make_golden.py captures
# under the same settings.  Set before torch is imported.
CPU_ARITHMETIC_ENV = {"ATEN_CPU_CAPABILITY": "avx512", "MKL_CBWR": "COMPATIBLE", "ONEDNN_MAX_CPU_ISA": "AVX512_CORE"}
CPU_THREADS = 8
os.environ.update(CPU_ARITHMETIC_ENV)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(CPU_THREADS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "f16x2_forward: backward test that keeps the default (f16x2) training forward")
    config.addinivalue_line("markers", "one_backward_leg: the test does not depend on the backward's matrix arithmetic (default leg only)")


def pytest_collection_modifyitems(config, items):
    """The tests of the shipped DEFAULT training arithmetic exist only under the split-f16 backward: their combination with the
    module fixture's fp32-backward leg is not a test (it used to be collected and skipped)."""
    keep, drop = [], []
    for it in items:
        f32_leg = "[dw_f32" in it.nodeid
        na = f32_leg and "default_arithmetic" in it.nodeid
        # tests whose subject does not depend on the backward's matrix arithmetic (no MLP backward in them, or HIP against HIP
        # on the same arithmetic) run under the default leg only: marker one_backward_leg
        na = na or (f32_leg and it.get_closest_marker("one_backward_leg") is not None)
        # the per-object launch forms of the super-batch test: both legs for the default form ("group"), one for the others
        na = na or (f32_leg and "test_render_backward_super_batch" in it.nodeid and not it.nodeid.endswith("-group]"))
        (drop if na else keep).append(it)
    if drop:
        config.hook.pytest_deselected(items=drop)
        items[:] = keep


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        if name not in cache:
            with np.load(os.path.join(GOLDEN, name + ".npz")) as f:
                cache[name] = {k: f[k] for k in f.files}
        return cache[name]

    return load
