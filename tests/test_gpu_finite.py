"""
The NaN / Inf monitor on the GPU (csrc/finite.hip, include/pnyolo.h pny_finite_*, util.FiniteMonitor):
  * sweep: tensors of 0 .. 4099 elements, as whole allocations and as slices that start one element in (4-byte alignment only),
    one value planted at the first and last element and on either side of the head / body / tail seams (and of the chunk
    seam): quiet NaN, negative NaN, the NaN 0x7f800001, +Inf, -Inf.  `bits` is what torch.isnan(t).any() / torch.isinf(t).any()
    give, `first` the lowest planted table index; every case has a group of its own and the words are read once;
  * +-FLT_MAX, the smallest denormal and -0 flag nothing, and a clean scan leaves the words exactly as reset left them;
  * flags are sticky across a clean check and clear on reset; groups do not leak; two runs give identical words;
  * a registered table of 70 tensors against immediate calls on the same data;
  * FiniteMonitor: names, re-registration when a watched buffer moves, one read per report;
  * no hidden waiting: check and reset calls return while their stream is still busy.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import DEV
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd.util import FiniteMonitor

pytestmark = pytest.mark.gpu

I32_MAX = 2 ** 31 - 1
COUNTS = (0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 4099)
CHUNK = 4096       # elements per workgroup (csrc/pny_finite.h FINITE_CHUNK): 4099 crosses it
PLANTS = {"qnan": 0x7fc00000, "neg_nan": 0xffc00000 - 2 ** 32, "snan_1": 0x7f800001, "pinf": 0x7f800000, "ninf": 0xff800000 - 2 ** 32}
# never flagged: +-FLT_MAX, the smallest denormal (both signs), -0, 0, ordinary values, the largest denormal
CLEAN = np.array([0x7f7fffff, 0xff7fffff - 2 ** 32, 0x00000001, 0x80000001 - 2 ** 32, 0x80000000 - 2 ** 32, 0, 0x3f800000, 0xc0490fdb - 2 ** 32,
                  0x007fffff], dtype=np.int64).astype(np.int32)


def clean_bits(n, seed):
    return torch.from_numpy(CLEAN[np.random.RandomState(seed).randint(0, len(CLEAN), size=n)])


def on_device(bits_i32, sliced):
    """int32 bit patterns -> fp32 tensor on the GPU: a whole allocation, or a slice starting one element into one."""
    n = bits_i32.numel()
    if not sliced:
        t = bits_i32.to(DEV).view(torch.float32)
        assert n == 0 or t.data_ptr() % 16 == 0
        return t
    base = torch.zeros(n + 1, dtype=torch.int32)
    base[1:] = bits_i32
    t = base.to(DEV).view(torch.float32)[1:]
    assert (n == 0 or t.data_ptr() % 16 == 4) and t.is_contiguous()
    return t


def seams(n, sliced):
    """Positions at the ends and on either side of the head / body / tail seams of finite.hip's split, and of the chunk seam."""
    mis = 1 if sliced else 0
    head = min((4 - mis) & 3, n)
    body = (n - head) & ~3
    pos = {0, n - 1, head - 1, head, head + body - 1, head + body, CHUNK - 1, CHUNK, CHUNK + 3 - mis, CHUNK + 4 - mis}
    return sorted(p for p in pos if 0 <= p < n)


def new_flags(groups):
    f = torch.full((groups, 2), -5, device=DEV, dtype=torch.int32)
    plib.check(plib.load().pny_finite_reset(C.c_void_p(f.data_ptr()), groups, plib.stream_of(DEV)))
    return f


def check_now(flags, tensors, groups):
    n = len(tensors)
    plib.check(plib.load().pny_finite_check_tensors((C.c_void_p * max(n, 1))(*[t.data_ptr() for t in tensors]),
                                                    (C.c_int64 * max(n, 1))(*[t.numel() for t in tensors]), (C.c_int32 * max(n, 1))(*groups), n,
                                                    C.c_void_p(flags.data_ptr()), plib.stream_of(DEV)))


def expected_bits(t):
    return int(bool(torch.isnan(t).any())) * plib.FINITE_NAN + int(bool(torch.isinf(t).any())) * plib.FINITE_INF


# --------------------------------------------------------------------------- sweep
@pytest.mark.parametrize("sliced", [False, True], ids=["whole", "slice"])
@pytest.mark.parametrize("count", COUNTS)
def test_sweep(count, sliced):
    """Every (position, planted value) is a call of three tensors [clean, planted, planted] in a group of its own: bits as
    torch gives them for the planted tensor, first = 1."""
    clean = clean_bits(count, 100 + count)
    cases = [(p, k) for p in seams(count, sliced) for k in PLANTS]
    flags = new_flags(len(cases) + 1)
    d_clean = on_device(clean, sliced)
    want, keep = [], []
    for g, (p, k) in enumerate(cases):
        bits = clean.clone()
        bits[p] = PLANTS[k]
        t, t2 = on_device(bits, sliced), on_device(bits, not sliced)
        keep += [t, t2]
        check_now(flags, [d_clean, t, t2], [g, g, g])
        want.append([expected_bits(t), 1])
        assert want[-1][0] == (plib.FINITE_INF if k.endswith("inf") else plib.FINITE_NAN)
    check_now(flags, [d_clean, d_clean], [len(cases)] * 2)          # the clean data alone, last group
    want.append([0, I32_MAX])
    got = flags.cpu().tolist()
    bad = [(cases[i] if i < len(cases) else "clean", got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, "count %d: (position, value), got, want: %s" % (count, bad[:6])
    if count == 0:
        assert cases == [] and got == [[0, I32_MAX]]
    else:
        assert len(cases) >= 5 and expected_bits(d_clean) == 0


def test_extreme_finite_values_flag_nothing_and_a_clean_scan_writes_nothing():
    vals = torch.tensor([3.4028234663852886e38, -3.4028234663852886e38, 1.401298464324817e-45, -1.401298464324817e-45, -0.0, 0.0, 1.0],
                        device=DEV).repeat(1000)
    assert float(vals.abs().max()) == 3.4028234663852886e38 and bool((vals[2::7] > 0).all()) and expected_bits(vals) == 0
    flags = new_flags(3)
    assert flags.cpu().tolist() == [[0, I32_MAX]] * 3
    # words that reset did NOT write stay as they are: a clean scan writes nothing (no OR of 0, no MIN of the index)
    marked = torch.tensor([[0, I32_MAX], [4, 7], [0, I32_MAX]], device=DEV, dtype=torch.int32)
    check_now(marked, [vals, vals[1:], vals[:4099]], [1, 1, 1])
    assert marked.cpu().tolist() == [[0, I32_MAX], [4, 7], [0, I32_MAX]]


def test_sticky_reset_and_groups():
    rs = np.random.RandomState(7)
    a, b, c = (torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV) for n in (300, 5000, 77))
    flags = new_flags(4)
    b[4097] = float("inf")
    check_now(flags, [a, b, c], [0, 2, 3])
    assert flags.cpu().tolist() == [[0, I32_MAX], [0, I32_MAX], [2, 1], [0, I32_MAX]], "groups do not leak"
    b[4097] = 0.0
    check_now(flags, [a, b, c], [0, 2, 3])                      # a clean check: the flag stays
    assert flags.cpu().tolist()[2] == [2, 1]
    c[0] = float("nan")
    a[299] = float("-inf")
    check_now(flags, [c, a, a], [2, 2, 0])                      # NaN joins Inf in group 2, the lower index wins; group 0: index 2
    assert flags.cpu().tolist() == [[2, 2], [0, I32_MAX], [3, 0], [0, I32_MAX]]
    plib.check(plib.load().pny_finite_reset(C.c_void_p(flags.data_ptr()), 3, plib.stream_of(DEV)))     # 3 of the 4 groups
    flags[3, 0] = 9
    plib.check(plib.load().pny_finite_reset(C.c_void_p(flags.data_ptr()), 3, plib.stream_of(DEV)))
    assert flags.cpu().tolist() == [[0, I32_MAX]] * 3 + [[9, I32_MAX]]


def table_of_70():
    rs = np.random.RandomState(70)
    sizes = [0, 1, 5, 4099, 64, 8192, 12289, 3, 0, 257] * 7
    tensors = [on_device(clean_bits(n, 700 + i), sliced=bool(i % 2)) for i, n in enumerate(sizes)]
    planted = {9: float("nan"), 13: float("inf"), 36: float("-inf"), 46: float("nan"), 65: float("inf"), 69: float("nan")}
    for i, v in planted.items():
        tensors[i][int(rs.randint(0, tensors[i].numel()))] = v
    return tensors, [i % 3 for i in range(70)], planted


def test_registered_table_of_70_against_immediate_calls():
    L = plib.load()
    tensors, groups, planted = table_of_70()
    h = C.c_void_p()
    plib.check(L.pny_finite_create(C.byref(h), 0))
    try:
        for i, (t, g) in enumerate(zip(tensors, groups)):
            assert L.pny_finite_add_tensor(h, C.c_void_p(t.data_ptr()) if t.numel() else None, t.numel(), g) == i
        want = [[0, I32_MAX] for _ in range(3)]
        for i in sorted(planted):
            want[i % 3][0] |= expected_bits(tensors[i])
            want[i % 3][1] = min(want[i % 3][1], i)
        runs = []
        for _ in range(2):                                      # two runs, identical words
            flags = new_flags(3)
            plib.check(L.pny_finite_check(h, 0, 70, C.c_void_p(flags.data_ptr()), plib.stream_of(DEV)))
            runs.append(flags.cpu().tolist())
        assert runs[0] == runs[1] == want
        # the same data through immediate calls of 8: the same bits; `first` is the position inside a call there
        imm = new_flags(3)
        for lo in range(0, 70, 8):
            check_now(imm, tensors[lo:lo + 8], groups[lo:lo + 8])
        got = imm.cpu().tolist()
        assert [w[0] for w in got] == [w[0] for w in want]
        assert [w[1] for w in got] == [min(i % 8 for i in planted if i % 3 == g) for g in range(3)]
        # a registered range of 8 and the immediate call on those 8 tensors: the same words, up to the range's first index
        sub, one = new_flags(3), new_flags(3)
        plib.check(L.pny_finite_check(h, 62, 8, C.c_void_p(sub.data_ptr()), plib.stream_of(DEV)))
        check_now(one, tensors[62:70], groups[62:70])
        sub, one = sub.cpu().tolist(), one.cpu().tolist()
        assert [w[0] for w in sub] == [w[0] for w in one] and any(w[0] for w in sub)
        assert [w[1] - 62 if w[0] else w[1] for w in sub] == [w[1] for w in one]
        # a range of empty tensors only, and bad ranges
        empty = new_flags(1)
        plib.check(L.pny_finite_check(h, 8, 1, C.c_void_p(empty.data_ptr()), plib.stream_of(DEV)))
        assert empty.cpu().tolist() == [[0, I32_MAX]]
        assert L.pny_finite_check(h, 0, 71, C.c_void_p(empty.data_ptr()), plib.stream_of(DEV)) == -1
        assert L.pny_finite_check(h, -1, 2, C.c_void_p(empty.data_ptr()), plib.stream_of(DEV)) == -1
    finally:
        torch.cuda.synchronize()
        L.pny_finite_destroy(h)


# --------------------------------------------------------------------------- FiniteMonitor
def test_monitor_names_and_re_registration():
    rs = np.random.RandomState(11)
    params = [torch.nn.Parameter(torch.from_numpy(rs.randn(n).astype(np.float32)).to(DEV)) for n in (10, 5000, 3, 700)]
    names = ["p%d" % i for i in range(4)]
    mon = FiniteMonitor(("render", "targets", "grads"), DEV)
    mon.watch("grads", params, names, grads=True)
    clean = {"render": (False, False, None), "targets": (False, False, None), "grads": (False, False, None)}
    mon.check("grads")                                          # no .grad yet: nothing to scan
    assert mon.report() == clean
    for p in params[:3]:
        p.grad = torch.zeros_like(p)
    mon.check("grads")
    assert mon.report() == clean
    params[2].grad[1] = float("inf")
    params[1].grad[4999] = float("nan")
    mon.check("grads")
    assert mon.report() == dict(clean, grads=(True, True, "p1"))
    mon.reset()
    assert mon.report() == clean and mon.flags.cpu().tolist() == [[0, I32_MAX]] * 3
    # zero_grad(set_to_none=True), then new buffers elsewhere: the monitor follows them on its own
    held = [p.grad for p in params[:3]]                         # (kept alive, so that the new ones have other addresses)
    for p in params:
        p.grad = None
    for p in params[1:]:
        p.grad = torch.zeros_like(p)
    assert params[1].grad.data_ptr() != held[1].data_ptr()
    held[1][7] = float("nan")                                   # the old buffer is no longer watched
    params[3].grad[699] = float("-inf")
    mon.check("grads")
    assert mon.report() == dict(clean, grads=(False, True, "p3"))
    # immediate checks: position inside the call; other groups untouched
    r, t = torch.zeros(64, 3, 7, device=DEV), torch.zeros(64, 3, 6, device=DEV)
    t[63, 2, 5] = float("nan")
    mon.check("render", r)
    mon.check("targets", r, t)
    assert mon.report() == {"render": (False, False, None), "targets": (True, False, "targets[1]"), "grads": (False, True, "p3")}
    with pytest.raises(AssertionError):
        mon.check("render", *([r] * 9))
    with pytest.raises(AssertionError):
        mon.check("render", r.double())
    # a table grown by many re-registrations is started afresh at reset; the flags still work afterwards
    for k in range(40):
        params[0].grad = torch.zeros(10, device=DEV) if k % 2 else held[0]
        mon.check("grads")
    mon.reset()
    assert mon._rows <= 4
    params[0].grad[9] = float("nan")
    mon.check("grads")
    assert mon.report()["grads"] == (True, True, "p0")           # p3's -Inf is still in its buffer
    mon.close()


# --------------------------------------------------------------------------- no hidden waiting
def test_checks_and_reset_do_not_wait_for_their_stream():
    """A queue of large matrix products is enqueued first; registered and immediate checks and a reset must come back with that
    stream still busy -- stream.query(), no timing threshold -- and give the words of an undisturbed run."""
    tensors, groups, _ = table_of_70()
    mon = FiniteMonitor(("a", "b", "grads"), DEV)
    mon.watch("grads", tensors)

    def run():
        mon.reset()
        mon.check("grads")
        mon.check("a", *tensors[:8])
        mon.check("b", tensors[3])
        return mon.flags

    quiet = run().cpu().tolist()                                # (also loads the kernels and registers the table)
    assert quiet[2][0] == 3 and quiet[0][0] == 0
    m = torch.randn(8192, 8192, device=DEV)
    out = torch.empty_like(m)
    torch.mm(m, m, out=out)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(DEV)
    for _ in range(60):
        torch.mm(m, m, out=out)
    assert not stream.query(), "the queue of matrix products was too short to test anything"
    flags = run()
    still_busy = not stream.query()
    torch.cuda.synchronize()
    assert still_busy, "a check or reset call waited for the stream"
    assert flags.cpu().tolist() == quiet
    mon.close()
