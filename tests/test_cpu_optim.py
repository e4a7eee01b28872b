"""
The one-launch Adam optimizer (pixel_nerf_yolo_amd.optim.Adam, include/pnyolo.h pny_optim_*), checks that need no GPU: the C
ABI (declared, typed, exported, kernel in the gfx950 code object, ABI version unchanged), the constructor's refusals, the loud
failure on CPU tensors, state_dict interchange with torch.optim.Adam in both directions, and the fp64 restatement of Adam
that tests/test_gpu_optim.py measures the kernel against -- pinned here to torch.optim.Adam(foreach=False) run in fp64.
"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from host_tools import ROOT, built_lib, c99_program, header_code  # noqa: F401
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.optim import Adam


# --------------------------------------------------------------------------- the yardstick
def adam_fp64(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
    """One Adam step (torch.optim.Adam: no amsgrad, no maximize, coupled weight decay) restated on float64 tensors; `step` is
    the 1-based count of the step being taken.  Returns the new (p, m, v)."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float64
    beta1, beta2 = betas
    if weight_decay != 0:
        g = g + weight_decay * p
    m = m + (g - m) * (1 - beta1)
    v = v * beta2 + g * g * (1 - beta2)
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    p = p - (lr / bc1) * m / (v.sqrt() / (bc2 ** 0.5) + eps)
    return p, m, v


def gradients(rs, shape):
    """N(0, 1) x 10^U(-6, 0) per element: six decades of gradient magnitudes."""
    return rs.standard_normal(shape) * 10.0 ** rs.uniform(-6.0, 0.0, size=shape)


@pytest.mark.parametrize("weight_decay,decay", [(0.0, 1.0), (1e-2, 1.0), (0.0, 0.9), (1e-2, 0.9)])
def test_fp64_restatement_is_torch_adam(weight_decay, decay):
    """The yardstick is Adam and not a guess: ten steps of torch.optim.Adam(foreach=False) on float64 tensors against the
    restatement, parameters and both moments to 1e-15 relative."""
    rs = np.random.RandomState(11)
    shapes = [(1,), (3,), (4,), (511,), (64, 33)]
    ps = [torch.nn.Parameter(torch.from_numpy(0.05 * rs.standard_normal(s))) for s in shapes]
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    lr = 1e-4
    opt = torch.optim.Adam(ps, lr=lr, weight_decay=weight_decay, foreach=False)
    for t in range(1, 11):
        gs = [torch.from_numpy(gradients(rs, s)) for s in shapes]
        for p, g in zip(ps, gs):
            p.grad = g.clone()
        opt.param_groups[0]["lr"] = lr
        opt.step()
        mine = [adam_fp64(p, g, m, v, t, lr, weight_decay=weight_decay) for (p, m, v), g in zip(mine, gs)]
        for p, (q, m, v) in zip(ps, mine):
            st = opt.state[p]
            for got, ref in ((q, p.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                assert float((got - ref).abs().max()) <= 1e-15 * float(ref.abs().max())
        lr *= decay


# --------------------------------------------------------------------------- C ABI
def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    """(Declared, bound, exported, the version and the mirror's layout: tests/test_cpu_abi.py.)"""
    code = header_code()
    assert "typedef struct pny_optim pny_optim;" in code
    fields = re.search(r"typedef struct pny_adam_hyper \{(.*?)\} pny_adam_hyper;", code, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", fields).strip() == "double lr, beta1, beta2, eps, weight_decay; int64_t step;"


def test_library_exports_them_and_holds_the_kernel(built_lib, tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("check_store_hazard", os.path.join(ROOT, "tools", "check_store_hazard.py"))
    chk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(chk)
    if not os.path.exists(chk.OBJDUMP):
        pytest.skip("llvm-objdump not installed")
    objs = chk.code_objects(plib.LIB_PATH, str(tmp_path))
    assert objs, "no gfx950 code object in the library"
    syms = "".join(subprocess.run([chk.OBJDUMP, "--syms", o], capture_output=True, text=True).stdout for o in objs)
    assert re.search(r"F \.text\s.*adam_multi_kernel", syms), "adam_multi_kernel is not in the gfx950 code object"


def test_argument_errors_follow_the_convention(built_lib):
    """0 / negative status plus pny_last_error(); without a GPU pny_optim_create is the loud PNY_ERR_NOGPU."""
    import ctypes as C
    assert built_lib.pny_optim_create(None, 0) == -1 and b"pny_optim_create" in built_lib.pny_last_error()
    assert built_lib.pny_optim_add_tensor(None, None, None, None, 4) == -1
    hyper = plib.AdamHyper(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
    assert built_lib.pny_optim_adam_step(None, C.byref(hyper), None, 0, 1, None, None) == -1
    built_lib.pny_optim_destroy(None)
    if not torch.cuda.is_available():
        h = C.c_void_p()
        rc = built_lib.pny_optim_create(C.byref(h), 0)
        assert rc == -4 and b"no HIP device" in built_lib.pny_last_error()


def test_header_with_the_optimizer_is_plain_c(built_lib, tmp_path):
    run = c99_program(tmp_path, '#include "pnyolo.h"\n'
                      "int main(void) { pny_adam_hyper h; pny_optim* o = 0; h.step = 1; h.lr = 1e-3; (void)h;\n"
                      "  pny_optim_destroy(o); return pny_optim_create(0, 0) == PNY_ERR_ARG ? 0 : 1; }\n", link=True)()
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)


# --------------------------------------------------------------------------- the Python class
def params(seed=3):
    rs = np.random.RandomState(seed)
    return [torch.nn.Parameter(torch.from_numpy(rs.standard_normal(s).astype(np.float32))) for s in [(5, 3), (7,), (2, 2, 2)]]


@pytest.mark.parametrize("name", ["amsgrad", "maximize", "capturable", "differentiable", "foreach", "fused"])
def test_unsupported_arguments_are_refused_by_name(name):
    with pytest.raises(NotImplementedError, match=name):
        Adam(params(), lr=1e-3, **{name: True})
    opt = Adam(params(), lr=1e-3, **{name: False if name not in ("foreach", "fused") else None})   # torch's own defaults pass
    assert isinstance(opt, torch.optim.Optimizer)


def test_constructor_is_torch_adams():
    opt = Adam(params(), 2e-3, (0.8, 0.99), 1e-7, 1e-2)
    ref = torch.optim.Adam(params(), 2e-3, (0.8, 0.99), 1e-7, 1e-2)
    assert {k: v for k, v in opt.param_groups[0].items() if k != "params"} == \
           {k: v for k, v in ref.param_groups[0].items() if k != "params"}
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            Adam(params(), **bad)
    two = Adam([dict(params=params()[:1], lr=1e-2), dict(params=params()[1:])], lr=1e-3)
    assert [g["lr"] for g in two.param_groups] == [1e-2, 1e-3]
    sched = torch.optim.lr_scheduler.ExponentialLR(two, 0.5)
    sched.step()
    assert [g["lr"] for g in two.param_groups] == [5e-3, 5e-4]


def test_step_on_cpu_tensors_is_loud():
    ps = params()
    opt = Adam(ps, lr=1e-3)
    assert opt.step() is None        # no gradients: nothing to do, as torch
    for p in ps:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(plib.PnyError, match="no CPU path"):
        opt.step()
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, ps)) and not any(opt.state[p] for p in ps)


def torch_adam_after_three_steps(ps, **kw):
    opt = torch.optim.Adam(ps, **kw)
    rs = np.random.RandomState(17)
    for _ in range(3):
        for p in ps[:2]:            # (the last parameter never gets a gradient: it has no state)
            p.grad = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32))
        opt.step()
    return opt


def assert_same_state_dict(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert set(a["state"]) == set(b["state"])
    for i in a["state"]:
        assert set(a["state"][i]) == set(b["state"][i]) == {"step", "exp_avg", "exp_avg_sq"}
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert x.dtype == y.dtype and x.shape == y.shape and x.device == y.device and torch.equal(x, y), (i, k)


def test_torch_state_dict_loads_and_comes_back():
    """A state made by three real torch.optim.Adam steps (the reference's `_optim` file is such a state_dict) through
    torch.save / torch.load into this class: state_dict() returns the same keys and equal tensors, the moments are views of one
    flat allocation each, and `step` is the CPU float tensor of non-capturable torch Adam."""
    import io
    ps = params()
    ref = torch_adam_after_three_steps(ps, lr=3e-4, weight_decay=1e-3)
    buf = io.BytesIO()
    torch.save(ref.state_dict(), buf)
    buf.seek(0)
    opt = Adam(ps, lr=1.0)
    opt.load_state_dict(torch.load(buf, weights_only=True))
    assert_same_state_dict(opt.state_dict(), ref.state_dict())
    assert opt.param_groups[0]["lr"] == 3e-4 and set(opt.state_dict()["state"]) == {0, 1}
    s0, s1 = opt.state[ps[0]], opt.state[ps[1]]
    assert s0["step"].device.type == "cpu" and s0["step"].dtype == torch.float32 and float(s0["step"]) == 3.0
    for k in ("exp_avg", "exp_avg_sq"):
        assert s0[k].untyped_storage().data_ptr() == s1[k].untyped_storage().data_ptr()
        assert s0[k].shape == ps[0].shape and s0[k].data_ptr() % 256 == s1[k].data_ptr() % 256
    assert s0["exp_avg"].untyped_storage().data_ptr() != s0["exp_avg_sq"].untyped_storage().data_ptr()


def test_state_dict_loads_into_torch_adam():
    """The reverse direction: this class's state_dict() into torch.optim.Adam, which then steps on from it exactly as from its
    own state."""
    ps = params()
    ref = torch_adam_after_three_steps(ps, lr=3e-4)
    opt = Adam(ps, lr=3e-4)
    opt.load_state_dict(ref.state_dict())
    ps_a, ps_b = params(), params()
    a, b = torch.optim.Adam(ps_a, lr=1.0), torch.optim.Adam(ps_b, lr=1.0)
    a.load_state_dict(opt.state_dict())
    b.load_state_dict(ref.state_dict())
    assert_same_state_dict(a.state_dict(), b.state_dict())
    for p, q in zip(ps_a, ps_b):
        p.grad, q.grad = torch.full_like(p, 0.25), torch.full_like(q, 0.25)
    a.step()
    b.step()
    assert all(torch.equal(p, q) for p, q in zip(ps_a, ps_b))
    assert_same_state_dict(a.state_dict(), b.state_dict())
