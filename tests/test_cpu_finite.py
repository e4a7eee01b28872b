"""
The NaN / Inf monitor without a GPU (include/pnyolo.h pny_finite_*, util.FiniteMonitor): the header compiles as strict C99
with a program that uses every entry under its exact type, and every bad argument comes back as PNY_ERR_ARG before anything
is launched (the device pointers here are made up and never dereferenced; no call in this file is a valid scan).
"""
import ctypes as C

import pytest
import torch

from host_tools import built_lib, c99_program, header_text  # noqa: F401
from pixel_nerf_yolo_amd import util as putil

DEVP = 4096     # stands for a device pointer; never dereferenced by the host


def test_entries_are_declared_bound_and_exported():
    """The comment of the entries names the reference lines they replace (declared, bound, exported, the argument counts and
    the constants: tests/test_cpu_abi.py)."""
    hdr = header_text()
    block = hdr[hdr.index("NaN / Inf monitor"):hdr.index("typedef struct pny_finite pny_finite")]
    assert "YoloTrainer.py:" in block and "163-178" in block and "188-194" in block


C99_MAIN = r"""
#include <stdio.h>
#include "pnyolo.h"
int main(void) {
    pny_finite* f = NULL;
    const float* ptrs[1] = {NULL};
    int64_t counts[1] = {0};
    int32_t groups[1] = {0};
    int (*create)(pny_finite**, int) = pny_finite_create;
    void (*destroy)(pny_finite*) = pny_finite_destroy;
    int (*add)(pny_finite*, const float*, int64_t, int) = pny_finite_add_tensor;
    int (*check)(pny_finite*, int, int, int32_t*, pny_stream) = pny_finite_check;
    int (*now)(const float* const*, const int64_t*, const int32_t*, int, int32_t*, pny_stream) = pny_finite_check_tensors;
    int (*reset)(int32_t*, int, pny_stream) = pny_finite_reset;
    printf("%d %d %d %d\n", PNY_FINITE_NAN, PNY_FINITE_INF, PNY_FINITE_MAX_IMMEDIATE,
           (int)(create && destroy && add && check && now && reset && !f && !ptrs[0] && !counts[0] && !groups[0]));
    return 0;
}
"""


def test_header_compiles_as_strict_c99(built_lib, tmp_path):
    """Every entry has exactly the C type a host would write for it."""
    run = c99_program(tmp_path, C99_MAIN, link=True)()
    assert run.returncode == 0 and run.stdout.split() == ["1", "2", "8", "1"], (run.returncode, run.stdout, run.stderr)


def now(L, ptrs, counts, groups, n=None, flags=DEVP, arrays=True):
    k = len(ptrs)
    n = k if n is None else n
    if not arrays:
        return L.pny_finite_check_tensors(None, None, None, n, C.c_void_p(flags), None)
    return L.pny_finite_check_tensors((C.c_void_p * max(k, 1))(*ptrs), (C.c_int64 * max(k, 1))(*counts), (C.c_int32 * max(k, 1))(*groups), n,
                                      C.c_void_p(flags) if flags else None, None)


def test_bad_arguments_are_refused_before_any_launch(built_lib):
    L = built_lib
    nine = ([DEVP] * 9, [4] * 9, [0] * 9)
    assert now(L, *nine) == -1 and b"8" in L.pny_last_error()                       # n > 8
    assert now(L, [DEVP], [4], [0], n=-1) == -1
    assert now(L, [None], [4], [0]) == -1 and b"NULL" in L.pny_last_error()         # NULL with a count > 0
    assert now(L, [DEVP, None], [4, 1], [0, 0]) == -1 and b"NULL" in L.pny_last_error()
    assert now(L, [DEVP], [-1], [0]) == -1 and now(L, [DEVP], [4], [-1]) == -1 and b"negative" in L.pny_last_error()
    assert now(L, [DEVP + 2], [4], [0]) == -1 and b"aligned" in L.pny_last_error()
    assert now(L, [DEVP], [4], [0], flags=None) == -1 and now(L, [DEVP], [4], [0], flags=DEVP + 1) == -1 and b"flags_dev" in L.pny_last_error()
    assert now(L, [], [], [], n=1, arrays=False) == -1 and b"null" in L.pny_last_error()
    # reset
    assert L.pny_finite_reset(None, 2, None) == -1 and L.pny_finite_reset(C.c_void_p(DEVP + 2), 2, None) == -1
    assert L.pny_finite_reset(C.c_void_p(DEVP), -1, None) == -1
    # the handle's entries without a handle
    assert L.pny_finite_create(None, 0) == -1
    assert L.pny_finite_add_tensor(None, C.c_void_p(DEVP), 4, 0) == -1 and L.pny_finite_check(None, 0, 0, C.c_void_p(DEVP), None) == -1
    L.pny_finite_destroy(None)      # a no-op


def test_nothing_to_scan_is_legal_and_launches_nothing(built_lib):
    """n = 0, and tensors of count 0 (with or without a pointer): PNY_OK; there is no chunk, so no kernel is enqueued -- which
    is why this may run with made-up pointers, with or without a GPU."""
    L = built_lib
    assert now(L, [], [], [], n=0) == 0
    assert now(L, [None, DEVP], [0, 0], [0, 1]) == 0
    assert L.pny_finite_reset(C.c_void_p(DEVP), 0, None) == 0


def test_no_gpu_is_loud(built_lib):
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = C.c_void_p()
    assert built_lib.pny_finite_create(C.byref(h), 0) == -4 and b"no CPU path" in built_lib.pny_last_error()      # PNY_ERR_NOGPU
    with pytest.raises(RuntimeError, match="no CPU path"):
        putil.FiniteMonitor(("render", "grads"), None)
