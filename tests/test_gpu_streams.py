"""
The library's ordering between streams (-m gpu, real MI355X): include/pnyolo.h promises that a scene "may migrate between
streams" -- a call that arrives on another stream than the previous call on its scene is ordered behind it by the library
(csrc/dev_resource.h StreamOrder::enter / mark), pny_model_refresh orders itself behind every scene's last call and every
scene's next call behind itself, and the Python classes fork side streams from torch's current stream (model.py fork_streams /
join_streams, render.py _flush_stream, model.py _trunk_stream).  The rest of the suite drives all of this on the default stream,
where a missing wait cannot show.

Every test follows three rules:
  1. reference first, on ONE stream: the test's call sequence with data set B; its outputs are held to the float64 oracle under
     the route's existing bar (imported), and the run warms every workspace, so that no allocation falls into the window later;
  2. poison: the same sequence serially with data set A (other latents, other weights), so that everything a missing wait would
     read stale holds A's answer; asserted on the oracle alone: A's and B's outputs differ by at least 100 x the bar;
  3. streamed run with B: a timed spin (torch.cuda._sleep, SPIN = 5 x test_gpu_trunk.SPIN_CYCLES, about 50 ms) on the stream that
     goes first, an event right behind it, then the whole sequence across the streams with no host synchronisation and no
     wait_stream of the test's own (except where the ABI makes the caller responsible).  After the last call is enqueued the
     spin's event must still be pending -- the host finished inside the window, so the library's waits, and not luck or a hidden
     synchronisation, produced the order -- and after a synchronise the outputs must be bit-equal to rule 1's.
A second, SHORT spin (1 x SPIN_CYCLES) stands in front of the work of a stream that must wait for the first one: it holds that
stream past the host's enqueue time, and ends 40 ms before the first stream's spin does, so that without the library's wait the
second stream's work runs well BEFORE the work it should have followed (a long spin there would hide the missing wait).

The streams come from a module fixture that proves with torch alone that the three it hands out run concurrently pairwise
(otherwise every test here would pass vacuously); it fails, and does not skip, when no such three exist.

ABI-level cases: a model of K = 128, 3 blocks (2 per view), 2 views, latent 8 x 8, 130 query points (two 64-sample tiles and a
ragged third), through the harness of test_gpu_projection.py; each with an F32 scene and with an AUTO scene whose projection is
ON (the split-f16 route and its projected-map cache).  Python-level cases: the public classes on a user side stream.
"""
import ctypes as C
import itertools
import time

import numpy as np
import pytest
import torch

import pnyolo_oracle as orc
import projection_ref as pr
from pixel_nerf_yolo_amd import lib as plib
from pixel_nerf_yolo_amd import synth
from test_cpu_optim import adam_fp64
from test_gpu_optim import within_bar
from test_gpu_parity import TOL
from test_gpu_projection import Model, dev
from test_gpu_trunk import SPIN_CYCLES, oracle_state, oracle_trunk

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F64 = torch.float32, torch.float64
SPIN, SHORT = 5, 1                 # x SPIN_CYCLES: the window, and the hold in front of a stream that must wait (module docstring)
POISON = 100.0                     # rule 2: A and B differ by at least this many bars
K, NVB, NB, NS, HL, WL, NQ = 128, 2, 3, 2, 8, 8, 130
IMG_W = IMG_H = 32                 # the target frame of the harness's cameras (test_gpu_projection.Model.scene)
LEGS = {"f32": ("f32", None), "auto_projected": ("auto", "on")}
HOST_MS = {}                       # test -> host issue time inside its window (test_zz_report prints the largest)
CHOSEN = {}


# ------------------------------------------------------------------------------------------------ streams that run concurrently
class Streams:
    def __init__(self, s1, s2, s3, s4, names):
        self.s1, self.s2, self.s3, self.s4, self.names = s1, s2, s3, s4, names


@pytest.fixture(scope="module")
def streams():
    """Three of up to 8 torch streams that run concurrently pairwise, shown by a torch-only control (on sa: spin, then fill a
    zeroed buffer with ones; on sb, with no wait: clone it; concurrent iff the clone is all zero), both ways for every pair;
    s4 is one more stream of the pool (concurrent with the three if there is one), for calls that only have to be elsewhere."""
    pool = [torch.cuda.Stream(DEV) for _ in range(8)]
    buf = torch.zeros(1 << 16, device=DEV)
    memo = {}

    def concurrent(i, j):
        if (i, j) not in memo:
            buf.zero_()
            torch.cuda.synchronize()
            with torch.cuda.stream(pool[i]):
                torch.cuda._sleep(SPIN_CYCLES)
                buf.fill_(1)
            with torch.cuda.stream(pool[j]):
                seen = buf.clone()
            torch.cuda.synchronize()
            memo[i, j] = bool((seen == 0).all())
        return memo[i, j]

    def pairwise(idx):
        return all(concurrent(a, b) for a, b in itertools.permutations(idx, 2))

    for tri in itertools.combinations(range(len(pool)), 3):
        if pairwise(tri):
            rest = [i for i in range(len(pool)) if i not in tri]
            fourth = next((i for i in rest if pairwise(tri + (i,))), rest[0])
            CHOSEN["streams"] = "streams %s of 8 created (creation order), the fourth: %d" % (list(tri), fourth)
            print("STREAMS fixture: " + CHOSEN["streams"])
            return Streams(*[pool[i] for i in tri + (fourth,)], names=tri + (fourth,))
    pytest.fail("no three of 8 torch streams run concurrently pairwise on this device (pairs that do: %s): every test of this "
                "module would pass whatever the library does" % sorted(p for p, ok in memo.items() if ok))


class Serial:
    """Rules 1 and 2: every stream of the sequence is torch's current (default) stream, and nothing spins."""

    def __init__(self):
        self.s1 = self.s2 = self.s3 = self.s4 = torch.cuda.current_stream(torch.device(DEV))

    def spin(self, stream, k=SPIN):
        pass


class Window:
    """Rule 3: the streams of the fixture; the first spin opens the window and its event closes it."""

    def __init__(self, streams):
        self.s1, self.s2, self.s3, self.s4 = streams.s1, streams.s2, streams.s3, streams.s4
        self.event = None
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()

    def spin(self, stream, k=SPIN):
        with torch.cuda.stream(stream):
            torch.cuda._sleep(k * SPIN_CYCLES)
        if self.event is None:
            assert k == SPIN
            self.event = torch.cuda.Event()
            self.event.record(stream)

    def close(self, what):
        """After the last call is enqueued: the first spin is still running.  Then wait for everything."""
        pending = not self.event.query()
        host_ms = 1e3 * (time.perf_counter() - self.t0)
        torch.cuda.synchronize()
        HOST_MS[what] = host_ms
        print("STREAMS %s: the host enqueued the sequence in %.2f ms, inside a spin of %d x SPIN_CYCLES" % (what, host_ms, SPIN))
        assert pending, ("%s: the spin had ended when the last call was enqueued (host time %.2f ms): the order may be luck, or "
                         "a call synchronised with the device" % (what, host_ms))


def cur():
    return torch.cuda.current_stream(torch.device(DEV))


def sp(stream):
    return C.c_void_p(stream.cuda_stream)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def metric(kind, got, ref):
    """abs: max |got - ref|; rel: over the reference's max (projection_ref.err)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    e = float(np.abs(got - ref).max())
    return e if kind == "abs" else e / float(np.abs(ref).max())


def three_rules(what, streams, outs, sequence, want, data_a, data_b, after=None):
    """outs: name -> (shape, bar, 'abs' | 'rel'); bar None: bit equality only (what `after` checks on the reference run).
    sequence(d, S, out): prepares (serially, synchronised) and returns the function that enqueues the calls on S's streams.
    want(d): name -> float64 oracle result.  after(out, d): called on a finished run, may add tensors to `out`.
    Returns the reference run's outputs."""
    def run(d, S):
        out = {k: torch.full(shape, float("nan"), device=DEV, dtype=F32) for k, (shape, _, _) in outs.items()}
        enqueue = sequence(d, S, out)
        torch.cuda.synchronize()
        if isinstance(S, Window):
            S.t0 = time.perf_counter()
        enqueue()
        if isinstance(S, Window):
            S.close(what)
        torch.cuda.synchronize()
        if after is not None:
            after(out, d)
        return out
    # 1. reference on one stream, against float64
    ref = run(data_b, Serial())
    w_b, w_a = want(data_b), want(data_a)
    for k, (_, bar, kind) in outs.items():
        if bar is None:
            continue
        e = metric(kind, ref[k].cpu().numpy(), w_b[k])
        print("STREAMS %s %-8s single stream vs float64: %.3e (bar %.1e)" % (what, k, e, bar))
        assert e < bar, (what, k, e, bar)
        # 2. ... and what the poison leaves behind is far from it
        gap = metric(kind, w_a[k], w_b[k])
        assert gap >= POISON * bar, (what, k, "data sets A and B are too close for a stale read to show", gap, bar)
    run(data_a, Serial())
    # 3. across the streams, behind the spin
    got = run(data_b, Window(streams))
    bad = [k for k in ref if not same_bits(got[k], ref[k])]
    assert not bad, "%s: %s differ from the single-stream run (max |difference| %s)" % (
        what, bad, ["%.3e" % float((got[k] - ref[k]).abs().nan_to_num(nan=float("inf")).max()) for k in bad])
    return ref


# ------------------------------------------------------------------------------------------------ the ABI rig and its data
def mlp_states(seed, k=K):
    sd = {}
    for f, pre in enumerate(("mlp_coarse.", "mlp_fine.")):
        sd.update(synth.mlp_state(seed + f, d_latent=k, n_blocks=NB, combine_layer=NVB, prefix=pre))
    return sd


def points(seed, n=NQ):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-0.3, 0.3, size=(n, 3)).astype(np.float32)
    vd = rs.standard_normal((n, 3)).astype(np.float32)
    return xyz, (vd / np.linalg.norm(vd, axis=1, keepdims=True)).astype(np.float32)


PTS = [points(9001), points(9002), points(9003)]
_DATA, _ORACLE = {}, {}


def data(tag, k=K):
    """Data set 'A' or 'B': three latents and three sets of MLP weights (host arrays)."""
    if (tag, k) not in _DATA:
        base = {"A": 9100, "B": 9200}[tag] + k
        _DATA[tag, k] = dict(tag=tag, k=k, lat=[synth.latent(base + i, NS, k, HL, WL) for i in range(3)],
                             w=[mlp_states(base + 10 + 10 * i, k) for i in range(3)])
    return _DATA[tag, k]


def oracle_query(state, lat, pts, width=IMG_W, height=IMG_H, key=None):
    """pny_query (coarse MLP) of the rig's scene in float64: (n, 4) numpy."""
    if key is not None and key in _ORACLE:
        return _ORACLE[key]
    mc = {n[len("mlp_coarse."):]: v for n, v in state.items() if n.startswith("mlp_coarse.")}
    mf = {n[len("mlp_fine."):]: v for n, v in state.items() if n.startswith("mlp_fine.")}
    poses, _ = synth.scene_cameras(lat.shape[0])
    sc = orc.Scene(mc, mf, lat, poses, torch.tensor(28.8), torch.tensor([[16.0, 16.0]]), width, height, n_blocks=NB,
                   combine_layer=NVB, dtype=F64)
    with torch.no_grad():
        out = orc.query(sc, pts[0], pts[1], coarse=True).numpy()
    if key is not None:
        _ORACLE[key] = out
    return out


def q(d, wi, li, pi):
    """Oracle query of data set d with its weights wi, latent li, on point set pi (memoised)."""
    return oracle_query(d["w"][wi], d["lat"][li], PTS[pi], key=(d["tag"], d["k"], wi, li, pi))


class Rig:
    """One model through the ABI with every MLP tensor bound on the device, and its scenes."""

    def __init__(self, leg, n_scenes=1, k=K, extra_state=None, frame=(IMG_W, IMG_H)):
        self.k, self.leg, self.frame = k, leg, frame
        self.m = Model(k, NVB, pr.weights(k, NVB), n_blocks=NB)
        self.m.state = dict(mlp_states(9000, k), **(extra_state or {}))
        self.L = self.m.L
        self.m.finalize()
        self.params = self.m.bind_all()
        self.mlp_names = [n for n in self.params if n.startswith("mlp_")]
        self.scenes = [self.scene() for _ in range(n_scenes)]
        self.pts = [(dev(x), dev(v)) for x, v in PTS]
        self._dev = {}
        torch.cuda.synchronize()

    def scene(self):
        s = C.c_void_p()
        plib.check(self.L.pny_scene_create(C.byref(s), self.m.h))
        self.m.scenes.append(s)
        prec, proj = LEGS[self.leg]
        plib.check(self.L.pny_scene_set_precision(s, plib.PRECISION[prec]))
        poses, _ = synth.scene_cameras(NS)
        focal, c = np.array([[28.8, 28.8]], dtype=np.float32), np.array([[16.0, 16.0]], dtype=np.float32)
        plib.check(self.L.pny_scene_set_cameras(s, np.ascontiguousarray(poses, dtype=np.float32).ctypes.data_as(C.c_void_p), NS,
                                                focal.ctypes.data_as(C.c_void_p), 1, c.ctypes.data_as(C.c_void_p), 1, *self.frame))
        if proj:
            plib.check(self.L.pny_scene_set_projection(s, plib.PROJECTION[proj]))
        return s

    def on_dev(self, d, kind, i):
        """Device copies of a data set's latent i / weights i, made once."""
        key = (d["tag"], kind, i)
        if key not in self._dev:
            self._dev[key] = dev(d["lat"][i]) if kind == "lat" else {n: dev(d["w"][i][n]) for n in self.mlp_names}
        return self._dev[key]

    # serial preparation, on the current stream
    def load(self, d, wi, into=None):
        """The bound parameter tensors (or the tensors `into`) take weights wi of the data set."""
        for n, t in self.on_dev(d, "w", wi).items():
            (into or self.params)[n].copy_(t)

    def bind(self, tensors):
        for n in self.mlp_names:
            plib.check(self.L.pny_model_bind_param(self.m.h, n.encode(), plib.ptr(tensors[n])))

    # the calls under test, on a given stream
    def set_latent(self, s, lat, st):
        plib.check(self.L.pny_scene_set_latent(s, plib.ptr(lat), lat.shape[0], lat.shape[1], lat.shape[2], lat.shape[3], sp(st)))

    def get_latent(self, s, out, st):
        plib.check(self.L.pny_scene_get_latent(s, plib.ptr(out), sp(st)))

    def project(self, s, st):
        plib.check(self.L.pny_scene_project(s, sp(st)))

    def projection(self, s, out, st):
        route = C.c_int(0)
        plib.check(self.L.pny_scene_projection(s, 0, plib.ptr(out), out.numel(), C.byref(route), sp(st)))
        return route.value

    def query(self, s, pi, out, st):
        xyz, vd = self.pts[pi]
        plib.check(self.L.pny_query(s, plib.ptr(xyz), plib.ptr(vd), xyz.shape[0], 1, plib.ptr(out), sp(st)))

    def refresh(self, st):
        plib.check(self.L.pny_model_refresh(self.m.h, sp(st)))

    def close(self):
        self.m.close()


@pytest.fixture
def rig(request):
    made = []

    def make(*a, **kw):
        made.append(Rig(*a, **kw))
        return made[-1]
    yield make
    for r in made:
        r.close()


QOUT = ((NQ, 4), TOL, "abs")       # a query's output: sigmoid rgb and relu sigma under the forward routes' bar


# ------------------------------------------------------------------------------------------------ handover of a scene's state
@pytest.mark.parametrize("leg", list(LEGS))
def test_latent_handover(leg, rig, streams):
    """pny_scene_set_latent on s1 behind the spin, pny_query on s2: the query reads the new latent."""
    r = rig(leg)
    s = r.scenes[0]

    def sequence(d, S, out):
        lat = r.on_dev(d, "lat", 0)

        def enqueue():
            S.spin(S.s1)
            r.set_latent(s, lat, S.s1)
            S.spin(S.s2, SHORT)
            r.query(s, 0, out["q"], S.s2)
        return enqueue
    w0 = r.m.state
    three_rules("latent_handover[%s]" % leg, streams, {"q": QOUT}, sequence,
                lambda d: {"q": oracle_query(w0, d["lat"][0], PTS[0], key=("w9000", d["tag"], 0, 0))}, data("A"), data("B"))


@pytest.mark.parametrize("leg", list(LEGS))
def test_projected_map_handover(leg, rig, streams):
    """pny_scene_set_latent and pny_scene_project on s1 behind the spin, pny_query on s2: the query reads the maps projected from
    the new latent (the AUTO leg: the scene's cached split-f16 maps)."""
    r = rig(leg)
    s = r.scenes[0]

    def sequence(d, S, out):
        lat = r.on_dev(d, "lat", 1)

        def enqueue():
            S.spin(S.s1)
            r.set_latent(s, lat, S.s1)
            r.project(s, S.s1)
            S.spin(S.s2, SHORT)
            r.query(s, 1, out["q"], S.s2)
        return enqueue
    w0 = r.m.state
    three_rules("projected_map_handover[%s]" % leg, streams, {"q": QOUT}, sequence,
                lambda d: {"q": oracle_query(w0, d["lat"][1], PTS[1], key=("w9000", d["tag"], 1, 1))}, data("A"), data("B"))
    if leg == "auto_projected":
        projected = C.c_int(-1)
        plib.check(r.L.pny_scene_last_mlp_stats(s, None, None, None, None, C.byref(projected)))
        assert projected.value == 1


@pytest.mark.parametrize("leg", list(LEGS))
def test_projection_read_out_handover(leg, rig, streams):
    """pny_scene_set_latent on s1 behind the spin, the read-out pny_scene_projection on s2: the maps of the new latent, under
    the read-out's own bar (projection_ref.bar of the route it reports)."""
    r = rig(leg)
    s = r.scenes[0]
    npix, route = NS * HL * WL, {}
    case = dict(K=K, kind="ordinary")

    def sequence(d, S, out):
        lat = r.on_dev(d, "lat", 2)

        def enqueue():
            S.spin(S.s1)
            r.set_latent(s, lat, S.s1)
            S.spin(S.s2, SHORT)
            route["code"] = r.projection(s, out["map"], S.s2)
        return enqueue
    w = np.concatenate([r.m.state["mlp_coarse.lin_z.%d.weight" % b] for b in range(NVB)])      # (NVB 512, K): block b's rows
    bar = pr.bar(case, "fallback")       # 128 pixels: below the tiled routes on either scene (asserted below)
    three_rules("projection_read_out[%s]" % leg, streams, {"map": ((npix, NVB * pr.HID), bar, "rel")}, sequence,
                lambda d: {"map": pr.project64(pr.rows_of(d["lat"][2]), w)}, data("A"), data("B"))
    assert pr.route_name(route["code"]) == "fallback"


@pytest.mark.parametrize("leg", list(LEGS))
def test_three_hops(leg, rig, streams):
    """s1 -> s2 -> s1 on one scene, which re-records the scene's one order event:
      s1: spin, pny_scene_set_latent(L0);
      s2: short spin, pny_query (reads L0: behind s1), then a FULL spin and pny_scene_get_latent (still L0);
      s1: pny_scene_set_latent(L1) (behind s2's read-out, which the second spin holds back), pny_query (reads L1).
    The spin goes on the stream that is left.  Every hop's output is checked."""
    r = rig(leg)
    s = r.scenes[0]

    def sequence(d, S, out):
        l0, l1 = r.on_dev(d, "lat", 0), r.on_dev(d, "lat", 1)

        def enqueue():
            S.spin(S.s1)
            r.set_latent(s, l0, S.s1)
            S.spin(S.s2, SHORT)
            r.query(s, 0, out["q0"], S.s2)
            S.spin(S.s2)
            r.get_latent(s, out["lat0"], S.s2)
            r.set_latent(s, l1, S.s1)
            r.query(s, 2, out["q1"], S.s1)
        return enqueue
    w0 = r.m.state
    three_rules("three_hops[%s]" % leg, streams, {"q0": QOUT, "lat0": ((NS, K, HL, WL), 1e-30, "abs"), "q1": QOUT}, sequence,
                lambda d: {"q0": oracle_query(w0, d["lat"][0], PTS[0], key=("w9000", d["tag"], 0, 0)), "lat0": d["lat"][0],
                           "q1": oracle_query(w0, d["lat"][1], PTS[2], key=("w9000", d["tag"], 1, 2))}, data("A"), data("B"))


# ------------------------------------------------------------------------------------------------ pny_model_refresh
@pytest.mark.parametrize("leg", list(LEGS))
def test_refresh_against_an_earlier_and_a_later_reader(leg, rig, streams):
    """Packed weights W0.  s1: spin, query Qa.  s2: short spin, pny_model_refresh with the parameters holding W1 (it must wait
    for Qa, which the spin on s1 still holds back).  s1: query Qb (it must wait for the refresh).  Qa carries W0's bits, Qb W1's."""
    r = rig(leg)
    s = r.scenes[0]

    def sequence(d, S, out):
        r.set_latent(s, r.on_dev(d, "lat", 0), cur())
        r.load(d, 0)
        r.refresh(cur())
        torch.cuda.synchronize()
        r.load(d, 1)

        def enqueue():
            S.spin(S.s1)
            r.query(s, 0, out["qa"], S.s1)
            S.spin(S.s2, SHORT)
            r.refresh(S.s2)
            r.query(s, 1, out["qb"], S.s1)
        return enqueue
    three_rules("refresh_readers[%s]" % leg, streams, {"qa": QOUT, "qb": QOUT}, sequence,
                lambda d: {"qa": q(d, 0, 0, 0), "qb": q(d, 1, 0, 1)}, data("A"), data("B"))
    # the refresh changes what a query returns by far more than the bar: Qa with W1's bits would not have passed
    assert metric("abs", q(data("B"), 1, 0, 0), q(data("B"), 0, 0, 0)) >= POISON * TOL


@pytest.mark.parametrize("leg", list(LEGS))
def test_refresh_with_two_scenes_of_one_model(leg, rig, streams):
    """Two scenes whose last calls sit on s1 and s3, each behind a spin; pny_model_refresh on s2 waits for both; one query per
    scene on a fourth stream reads the refreshed weights."""
    r = rig(leg, n_scenes=2)
    sa, sb = r.scenes

    def sequence(d, S, out):
        r.set_latent(sa, r.on_dev(d, "lat", 0), cur())
        r.set_latent(sb, r.on_dev(d, "lat", 1), cur())
        r.load(d, 0)
        r.refresh(cur())
        torch.cuda.synchronize()
        r.load(d, 1)

        def enqueue():
            S.spin(S.s1)
            r.query(sa, 0, out["a0"], S.s1)
            S.spin(S.s3)
            r.query(sb, 1, out["b0"], S.s3)
            S.spin(S.s2, SHORT)
            r.refresh(S.s2)
            S.spin(S.s4, SHORT)
            r.query(sa, 2, out["a1"], S.s4)
            r.query(sb, 0, out["b1"], S.s4)
        return enqueue
    three_rules("refresh_two_scenes[%s]" % leg, streams, {k: QOUT for k in ("a0", "b0", "a1", "b1")}, sequence,
                lambda d: {"a0": q(d, 0, 0, 0), "b0": q(d, 0, 1, 1), "a1": q(d, 1, 0, 2), "b1": q(d, 1, 1, 0)}, data("A"), data("B"))


ADAM_LR = 2e-2      # one step moves every weight by about lr: the stepped model's outputs are far from the unstepped one's


def adam_gradients(d, names):
    rs = np.random.RandomState(9300 + ord(d["tag"]))
    return {n: (1e-3 * rs.standard_normal(d["w"][0][n].shape)).astype(np.float32) for n in names}


def adam_stepped64(d, names):
    """Weights 0 of the data set after one Adam step at ADAM_LR on adam_gradients, in float64 (test_cpu_optim.adam_fp64)."""
    g = adam_gradients(d, names)
    out = {}
    for n in names:
        p = torch.from_numpy(d["w"][0][n]).double()
        out[n] = adam_fp64(p, torch.from_numpy(g[n]).double(), torch.zeros_like(p), torch.zeros_like(p), 1, ADAM_LR)[0]
    return out


@pytest.mark.parametrize("leg", list(LEGS))
def test_adam_step_refreshes_behind_a_pending_query(leg, rig, streams):
    """pny_optim_adam_step(..., model, s2): the step and the refresh it chains go on s2 while query Qa is pending on s1 behind
    the spin; Qb on s1 follows.  Qa carries the unstepped weights' bits, Qb the stepped ones'; the stepped parameters are held
    to float64 Adam under test_gpu_optim.py's bar (twice torch's own fp32 error plus an ulp) and are bit-equal across the runs."""
    r = rig(leg)
    s = r.scenes[0]
    names = r.mlp_names
    opt = C.c_void_p()
    plib.check(r.L.pny_optim_create(C.byref(opt), 0))
    moments = {n: (torch.zeros_like(r.params[n]), torch.zeros_like(r.params[n])) for n in names}
    for n in names:
        i = r.L.pny_optim_add_tensor(opt, plib.ptr(r.params[n]), plib.ptr(moments[n][0]), plib.ptr(moments[n][1]), r.params[n].numel())
        assert i >= 0
    hyper = plib.AdamHyper(lr=ADAM_LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, step=1)
    grads_dev = {}

    def sequence(d, S, out):
        g = grads_dev.setdefault(d["tag"], {n: dev(a) for n, a in adam_gradients(d, names).items()})
        table = (C.c_void_p * len(names))(*[g[n].data_ptr() for n in names])
        r.set_latent(s, r.on_dev(d, "lat", 0), cur())
        r.load(d, 0)
        for m_, v_ in moments.values():
            m_.zero_()
            v_.zero_()
        r.refresh(cur())

        def enqueue():
            S.spin(S.s1)
            r.query(s, 0, out["qa"], S.s1)
            S.spin(S.s2, SHORT)
            plib.check(r.L.pny_optim_adam_step(opt, C.byref(hyper), table, 0, len(names), r.m.h, sp(S.s2)))
            r.query(s, 1, out["qb"], S.s1)
        return enqueue

    def after(out, d):
        for n in names:
            out["p:" + n] = r.params[n].detach().clone()

    def want(d):
        stepped = {n: v.float().numpy() for n, v in adam_stepped64(d, names).items()}
        return {"qa": q(d, 0, 0, 0), "qb": oracle_query(stepped, d["lat"][0], PTS[1], key=("adam", d["tag"]))}
    try:
        ref = three_rules("adam_step[%s]" % leg, streams, {"qa": QOUT, "qb": QOUT}, sequence, want, data("A"), data("B"), after)
        # the reference run's parameters against float64 Adam, beside torch.optim.Adam's fp32 step on the same inputs
        d = data("B")
        exact = adam_stepped64(d, names)
        ps = [torch.nn.Parameter(dev(d["w"][0][n])) for n in names]
        for p, n in zip(ps, names):
            p.grad = grads_dev["B"][n].clone()
        torch.optim.Adam(ps, lr=ADAM_LR, foreach=False).step()
        e_k = max(float((ref["p:" + n].double().cpu() - exact[n]).abs().max()) for n in names)
        e_t = max(float((p.detach().double().cpu() - exact[n]).abs().max()) for p, n in zip(ps, names))
        within_bar("adam_step[%s] parameters" % leg, e_k, e_t, max(float(v.abs().max()) for v in exact.values()))
        assert metric("abs", want(d)["qb"], q(d, 0, 0, 1)) >= POISON * TOL      # the step is visible in what a query returns
    finally:
        torch.cuda.synchronize()
        r.L.pny_optim_destroy(opt)


@pytest.mark.parametrize("leg", list(LEGS))
def test_rebind_between_two_refreshes_on_a_side_stream(leg, rig, streams):
    """The job table of pny_model_refresh holds the parameters' device pointers and is rewritten in place after a
    pny_model_bind_param.  On s1: spin, refresh #1 (parameters bound to storage P_old), query Q1, every tensor re-bound to
    P_new (other values), refresh #2, query Q2.  Refresh #1's launch is still queued behind the spin when refresh #2 rewrites
    the table: Q1 must carry P_old's bits and Q2 P_new's.  Before the rewrite was ordered behind the last repack launch it was a
    blocking hipMemcpy, which waits for nothing on a non-blocking stream: measured on the MI355X with that upload put back, the
    host left the window after 0.15 ms and Q1 came out 2.085 from the single-stream run, which is exactly the distance between
    the oracle's Q1 on P_old's and on P_new's weights (both legs): refresh #1 had read P_new's pointers.
    Prepared serially: the table points at P_old while the packed weights still hold what the previous run left (rule 2's
    poison in the streamed run), so both refreshes of the window have work to do and only the second one uploads a table."""
    r = rig(leg)
    s = r.scenes[0]
    p_old = r.params
    p_new = {n: torch.empty_like(t) for n, t in p_old.items() if n in r.mlp_names}

    def sequence(d, S, out):
        r.set_latent(s, r.on_dev(d, "lat", 0), cur())
        r.bind(p_old)
        r.refresh(cur())          # uploads the table of P_old; packs whatever P_old held
        torch.cuda.synchronize()
        r.load(d, 0, p_old)
        r.load(d, 1, p_new)

        def enqueue():
            S.spin(S.s1)
            r.refresh(S.s1)
            r.query(s, 0, out["q1"], S.s1)
            r.bind(p_new)
            r.refresh(S.s1)
            r.query(s, 1, out["q2"], S.s1)
        return enqueue
    three_rules("rebind_between_refreshes[%s]" % leg, streams, {"q1": QOUT, "q2": QOUT}, sequence,
                lambda d: {"q1": q(d, 0, 0, 0), "q2": q(d, 1, 0, 1)}, data("A"), data("B"))
    assert metric("abs", q(data("B"), 1, 0, 0), q(data("B"), 0, 0, 0)) >= POISON * TOL       # Q1 on P_new's weights would fail


# ------------------------------------------------------------------------------------------------ with the ResNet-34 trunk
K_ENC = 512                        # the trunk's latent width
ENC_H, ENC_W = 32, 40              # the smallest shape of test_gpu_trunk.py: latent 16 x 20
_ENC = {}


def enc_state():
    if "sd" not in _ENC:
        _ENC["sd"] = synth.resnet34_state(9400, residual_gain=0.25)
    return _ENC["sd"]


def enc_data(tag):
    """Data set 'A' or 'B' of the trunk cases: 2 scenes x NS images, and two conv1 weights (P_old's and P_new's values)."""
    if tag not in _ENC:
        base = {"A": 9500, "B": 9600}[tag]
        conv = [synth.resnet34_state(base + i, residual_gain=0.25)["encoder.model.conv1.weight"] for i in range(2)]
        _ENC[tag] = dict(data(tag, K_ENC), images=synth.images(base + 7, 2 * NS, ENC_H, ENC_W), conv=conv)
    return _ENC[tag]


def test_trunk_rebind_between_two_forwards_on_a_side_stream(rig, streams):
    """pny_trunk_train_forward's pack-job table holds the conv weights' device pointers (csrc/encoder_train.hip
    trunk_upload_jobs): on s1, spin, forward #1 (conv1.weight bound to P_old), conv1.weight re-bound to P_new, forward #2.  The
    first forward's pack launch is still queued when the second rewrites the table.  Batch statistics, momentum 0 (the running
    statistics stay put, so every run starts from the same state); each latent under test_gpu_trunk.py's bar, 2e-4 x
    max(1, max |latent|), against the float64 trunk."""
    r = rig("f32", n_scenes=0, k=K_ENC, extra_state=enc_state())
    name = "encoder.model.conv1.weight"
    p_old, p_new = r.params[name], torch.empty_like(r.params[name])
    n = NS
    scratch = torch.empty(n, 512, ENC_H // 2, ENC_W // 2, device=DEV, dtype=F32)
    on_dev = {}

    def forward(images, out, st):
        plib.check(r.L.pny_trunk_train_forward(r.m.h, plib.ptr(images), n, ENC_H, ENC_W, 0.0, 0, plib.ptr(out), sp(st)))

    def sequence(d, S, out):
        img, c_old, c_new = on_dev.setdefault(d["tag"], (dev(d["images"][:n]), dev(d["conv"][0]), dev(d["conv"][1])))
        p_old.copy_(c_old)
        p_new.copy_(c_new)
        plib.check(r.L.pny_model_bind_param(r.m.h, name.encode(), plib.ptr(p_old)))
        forward(img, scratch, cur())       # uploads the table of P_old

        def enqueue():
            S.spin(S.s1)
            forward(img, out["lat1"], S.s1)
            plib.check(r.L.pny_model_bind_param(r.m.h, name.encode(), plib.ptr(p_new)))
            forward(img, out["lat2"], S.s1)
        return enqueue

    def want(d):
        if "trunk" + d["tag"] not in _ORACLE:
            res = []
            for c in d["conv"]:
                with torch.no_grad():
                    res.append(oracle_trunk(oracle_state(dict(enc_state(), **{name: c})), torch.from_numpy(d["images"][:n]), True,
                                            training=True).numpy())
            _ORACLE["trunk" + d["tag"]] = dict(lat1=res[0], lat2=res[1])
        return _ORACLE["trunk" + d["tag"]]
    w = want(enc_data("B"))
    shape = (n, 512, ENC_H // 2, ENC_W // 2)
    outs = {k: (shape, 2e-4 * max(1.0, float(np.abs(w[k]).max())), "abs") for k in ("lat1", "lat2")}
    three_rules("trunk_rebind", streams, outs, sequence, want, enc_data("A"), enc_data("B"))
    assert metric("abs", w["lat1"], w["lat2"]) >= POISON * outs["lat1"][1]        # forward #1 on P_new's weights would fail


@pytest.mark.parametrize("leg", list(LEGS))
def test_order_event_invalidated_by_a_refresh(leg, rig, streams):
    """pny_scenes_encode of two scenes on s1 leaves a marked stream point (an order event recorded right behind the encode,
    StreamOrder::mark); then, on s1, a spin and pny_model_refresh; then one query per scene on s2 and s3.  The queries must wait
    for the refresh and not for the marked point in front of it: they read the refreshed weights.  The queries' float64
    reference takes the scenes' latents as the library's inference trunk produced them (read out with pny_scene_get_latent in
    a serial run beforehand; the trunk itself is held to float64 in test_gpu_trunk.py)."""
    r = rig(leg, n_scenes=2, k=K_ENC, extra_state=enc_state(), frame=(ENC_W, ENC_H))
    arr = (C.c_void_p * 2)(*r.scenes)
    images, lat_gpu = {}, {}

    def encode(d, st):
        img = images.setdefault(d["tag"], dev(d["images"]))
        plib.check(r.L.pny_scenes_encode(arr, 2, plib.ptr(img), NS, ENC_H, ENC_W, sp(st)))
    for d in (enc_data("A"), enc_data("B")):
        encode(d, cur())
        got = [torch.empty(NS, 512, ENC_H // 2, ENC_W // 2, device=DEV, dtype=F32) for _ in r.scenes]
        for s, g in zip(r.scenes, got):
            r.get_latent(s, g, cur())
        torch.cuda.synchronize()
        lat_gpu[d["tag"]] = [g.cpu().numpy() for g in got]
    assert metric("abs", lat_gpu["A"][0], lat_gpu["B"][0]) > 0.1

    def sequence(d, S, out):
        r.load(d, 0)
        r.refresh(cur())
        torch.cuda.synchronize()
        r.load(d, 1)

        def enqueue():
            S.spin(S.s1)
            encode(d, S.s1)
            S.spin(S.s1)
            r.refresh(S.s1)
            S.spin(S.s2, SHORT)
            r.query(r.scenes[0], 0, out["q0"], S.s2)
            S.spin(S.s3, SHORT)
            r.query(r.scenes[1], 1, out["q1"], S.s3)
        return enqueue

    def want(d, wi=1):
        return {"q%d" % i: oracle_query(d["w"][wi], lat_gpu[d["tag"]][i], PTS[i], ENC_W, ENC_H, key=("enc", leg, d["tag"], wi, i))
                for i in range(2)}
    three_rules("order_event_invalidated[%s]" % leg, streams, {"q0": QOUT, "q1": QOUT}, sequence, want, enc_data("A"), enc_data("B"))
    stale = want(enc_data("B"), wi=0)
    assert all(metric("abs", stale[k], want(enc_data("B"))[k]) >= POISON * TOL for k in stale)      # the unrefreshed weights would fail


# ------------------------------------------------------------------------------------------------ the public classes on a user stream
# PixelNeRFNet / NeRFRenderer / optim.Adam follow torch's current stream (lib.stream_of) and fork their side streams from it
# (fork_streams, _flush_stream).  A model of 3 blocks (2 per view) at L = 512 on supplied latents of 8 x 8 that require grad, the
# default arithmetic (split-f16 forward and backward: the f16x2_default leg of test_gpu_grad_shapes.py, RTOL on relu-safe rays
# at its margin AMBIG_DEFAULT), 6 + 4 samples per ray (few, so that relu-safe rays exist at that margin; __graft_entry__.smoke).
# Rule 1's run is the step on the DEFAULT stream; rule 2's poison runs serially on the user stream (which also warms that
# stream's share of torch's allocator); rule 3 enqueues the spin on the user stream and the whole step behind it.
PY = dict(ns=2, H=32, W=32, hl=8, wl=8, nb=3, cl=2, kc=6, kf=4, kfd=2, near=0.3, far=1.8, lr=1e-3)
PY_SEED = {"A": 9700, "B": 9800}
_PY = {}


class _SlowIdentity(torch.autograd.Function):
    """Identity whose backward spins on the current stream before it writes its output (test_gpu_trunk.py): what consumes that
    gradient gets its input late."""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        torch.cuda._sleep(SPIN_CYCLES)
        return g.clone()


def py_weights(tag):
    kw = dict(d_latent=512, d_out=4, n_blocks=PY["nb"], combine_layer=PY["cl"])
    return synth.mlp_state(PY_SEED[tag] + 1, **kw), synth.mlp_state(PY_SEED[tag] + 2, **kw)


def py_latent(tag, SB):
    return np.concatenate([synth.latent(PY_SEED[tag] + 10 + i, PY["ns"], 512, PY["hl"], PY["wl"]) for i in range(SB)])


def py_poses(SB):
    return np.stack([synth.scene_cameras(PY["ns"], radius=1.3 + 0.1 * i)[0] for i in range(SB)]).astype(np.float32)


def py_scenes(tag, SB):
    """The oracle's float64 scenes of a data set: one per object on shared MLP leaves, each latent a leaf."""
    sd_c, sd_f = py_weights(tag)
    mc = {k: torch.from_numpy(v).to(F64).requires_grad_() for k, v in sd_c.items()}
    mf = {k: torch.from_numpy(v).to(F64).requires_grad_() for k, v in sd_f.items()}
    lat, poses, ns = py_latent(tag, SB), py_poses(SB), PY["ns"]
    scs = []
    for i in range(SB):
        sc = orc.Scene(mc, mf, lat[i * ns:(i + 1) * ns], poses[i], torch.tensor(0.9 * PY["W"]), torch.tensor([[PY["W"] * 0.5, PY["H"] * 0.5]]),
                       PY["W"], PY["H"], n_blocks=PY["nb"], combine_layer=PY["cl"], dtype=F64)
        sc.mlp_coarse, sc.mlp_fine = mc, mf
        sc.latent = torch.from_numpy(lat[i * ns:(i + 1) * ns]).to(F64).requires_grad_()
        scs.append(sc)
    return scs


def py_inputs(SB, B):
    """Rays (SB, B, 8), draws (SB B rows) and ground truth of a step: per object the first B rays of its target view that are
    relu-safe at AMBIG_DEFAULT on data set B's float64 oracle (the reference run's data)."""
    if ("in", SB, B) not in _PY:
        from helpers import clean_rays
        import test_gpu_grad_shapes as gs
        kc, kf, kfd = PY["kc"], PY["kf"], PY["kfd"]
        rs = np.random.RandomState(9900 + SB)
        scs, rays, drs = py_scenes("B", SB), [], []
        for i in range(SB):
            cand = orc.gen_rays(synth.pose_spherical(100.0 + 25 * i, -20.0, 1.3)[None], PY["W"], PY["H"], 0.9 * PY["W"], PY["near"],
                                PY["far"])[0].reshape(-1, 8)
            nc = cand.shape[0]
            dr = dict(u_coarse=rs.rand(nc, kc).astype(np.float32), u_fine=rs.rand(nc, kf - kfd).astype(np.float32),
                      u_fine2=rs.rand(nc, kf - kfd).astype(np.float32), g_depth=rs.randn(nc, kfd).astype(np.float32))
            keep = clean_rays(scs[i], cand, kc, kf, kfd, dr, B, ambig=gs.AMBIG_DEFAULT)
            rays.append(cand[torch.from_numpy(keep)])
            drs.append({k: v[keep] for k, v in dr.items()})
        gt = torch.from_numpy(rs.uniform(0, 1, size=(SB, B, 3)).astype(np.float32))
        _PY["in", SB, B] = dict(rays=torch.stack(rays), draws=drs, gt=gt)
    return _PY["in", SB, B]


def py_oracle(tag, SB, B):
    """float64 autograd through the oracle: rendered colours, every MLP parameter gradient, d loss / d latent."""
    if ("ref", tag, SB, B) not in _PY:
        inp, scs = py_inputs(SB, B), py_scenes(tag, SB)
        c, f = [], []
        for i, sc in enumerate(scs):
            d = inp["draws"][i]
            r = orc.render(sc, inp["rays"][i], PY["kc"], PY["kf"], PY["kfd"], d["u_coarse"], d["u_fine"], d["u_fine2"], d["g_depth"])
            c.append(r["coarse"]["rgb"])
            f.append(r["fine"]["rgb"])
        c, f, gt = torch.stack(c), torch.stack(f), inp["gt"].to(F64)
        (torch.nn.functional.mse_loss(c, gt) + torch.nn.functional.mse_loss(f, gt)).backward()
        mlps = (("mlp_coarse.", scs[0].mlp_coarse), ("mlp_fine.", scs[0].mlp_fine))
        grads = {pre + k: (v.grad if v.grad is not None else torch.zeros_like(v)) for pre, sd in mlps for k, v in sd.items()}
        _PY["ref", tag, SB, B] = dict(rgb_c=c.detach(), rgb_f=f.detach(), grads=grads, lat=torch.cat([sc.latent.grad for sc in scs]))
    return _PY["ref", tag, SB, B]


class Trainer:
    """One net, renderer and optimizer of the project; step() is one whole training step on torch's current stream."""

    def __init__(self, SB, B):
        from helpers import scene_pair
        from pixel_nerf_yolo_amd.optim import Adam
        from pixel_nerf_yolo_amd.render import NeRFRenderer
        self.SB, self.B = SB, B
        self.net, _ = scene_pair(PY["ns"], PY["H"], PY["W"], 512, 4, PY["nb"], PY["cl"], 9650, lat_hw=(PY["hl"], PY["wl"]))
        self.net.set_deterministic(True)          # as test_gpu_deterministic.py: the latent gradient's fixed-point sums
        self.ren = NeRFRenderer(n_coarse=PY["kc"], n_fine=PY["kf"], n_fine_depth=PY["kfd"], white_bkgd=True).train()
        self.params = dict(self.net.trainable_mlp_parameters())
        self.opt = Adam(list(self.params.values()), lr=PY["lr"], model=self.net)
        inp = py_inputs(SB, B)
        self.rays, self.gt = inp["rays"].to(DEV), inp["gt"].to(DEV)
        self.draws = {k: torch.from_numpy(np.concatenate([d[k] for d in inp["draws"]])).to(DEV) for k in inp["draws"][0]}
        self.images = torch.zeros(SB, PY["ns"], 3, PY["H"], PY["W"])
        self.poses, self.focal = torch.from_numpy(py_poses(SB)), torch.tensor(0.9 * PY["W"])
        self.cc = torch.tensor([[PY["W"] * 0.5, PY["H"] * 0.5]])
        self.w_dev = {t: {pre + k: torch.from_numpy(v).to(DEV) for pre, sd in zip(("mlp_coarse.", "mlp_fine."), py_weights(t)) for k, v in sd.items()}
                      for t in "AB"}
        self.lat_dev = {t: torch.from_numpy(py_latent(t, SB)).to(DEV) for t in "AB"}
        self.call = None                          # bind_parallel's wrapper, when a test sets one
        torch.cuda.synchronize()

    def prepare(self, tag):
        """Serially: the data set's weights into the parameters (in place), the optimizer back at step 0, a fresh latent leaf."""
        with torch.no_grad():
            for n, p in self.params.items():
                p.copy_(self.w_dev[tag][n])
        for st in self.opt.state.values():
            if st:
                st["step"].zero_()
                st["exp_avg"].zero_()
                st["exp_avg_sq"].zero_()
        self.opt.zero_grad(set_to_none=True)
        self.lat = self.lat_dev[tag].clone().requires_grad_()
        self.out = None
        torch.cuda.synchronize()

    def encode(self):
        self.net.encode(self.images, self.poses, self.focal, c=self.cc, latent=self.lat)

    def render_and_step(self):
        self.ren.draws = self.draws
        out = self.call(self.rays, want_weights=True) if self.call else self.ren(self.net, self.rays, want_weights=True)
        c, f = _SlowIdentity.apply(out["coarse"]["rgb"]), _SlowIdentity.apply(out["fine"]["rgb"])     # the backward's inputs come late
        (torch.nn.functional.mse_loss(c, self.gt) + torch.nn.functional.mse_loss(f, self.gt)).backward()
        self.opt.step()
        self.out = out

    def collect(self):
        torch.cuda.synchronize()
        res = {"rgb_c": self.out["coarse"]["rgb"].detach().clone(), "rgb_f": self.out["fine"]["rgb"].detach().clone(),
               "lat": self.lat.grad.detach().clone()}
        for n, p in self.params.items():
            res["g:" + n] = p.grad.detach().clone()
            res["w:" + n] = p.detach().clone()
        return res


def py_window(what, user, enqueue):
    """Rule 3 for the Python-level cases: the spin and its event on `user`, then enqueue(); the window assertion."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(user):
        torch.cuda._sleep(SPIN * SPIN_CYCLES)
        ev = torch.cuda.Event()
        ev.record()
    enqueue()
    pending = not ev.query()
    host_ms = 1e3 * (time.perf_counter() - t0)
    torch.cuda.synchronize()
    HOST_MS[what] = host_ms
    print("STREAMS %s: the host enqueued the sequence in %.2f ms, inside a spin of %d x SPIN_CYCLES" % (what, host_ms, SPIN))
    assert pending, "%s: the spin had ended when the last call was enqueued (host time %.2f ms)" % (what, host_ms)


def check_training_reference(what, T, ref):
    """Rule 1 for a training step (the default-stream run `ref` of data set B) and rule 2's condition, on the oracle."""
    from helpers import RTOL, grad_check
    o_b, o_a = py_oracle("B", T.SB, T.B), py_oracle("A", T.SB, T.B)
    for k in ("rgb_c", "rgb_f"):
        e = metric("abs", ref[k].cpu().numpy(), o_b[k].numpy())
        print("STREAMS %s %s vs float64: %.3e (bar %.1e)" % (what, k, e, TOL))
        assert e < TOL, (what, k, e)
        assert metric("abs", o_a[k].numpy(), o_b[k].numpy()) >= POISON * TOL
    worst = 0.0
    for n, g in o_b["grads"].items():
        worst = max(worst, grad_check(n, ref["g:" + n], g.float(), RTOL))
        assert metric("rel", o_a["grads"][n].numpy(), g.numpy()) >= POISON * RTOL, (what, n)
    e_lat = grad_check("latent", ref["lat"], o_b["lat"].float(), RTOL)
    assert metric("rel", o_a["lat"].numpy(), o_b["lat"].numpy()) >= POISON * RTOL
    print("STREAMS %s gradients vs float64: parameters %.2e, latent %.2e of the tensor's max (bar %.1e)" % (what, worst, e_lat, RTOL))
    # the stepped weights against float64 Adam on the run's own fp32 gradients, beside torch's fp32 Adam (test_gpu_optim.py's rule)
    e_k = e_t = big = 0.0
    for n in T.params:
        p0, g = T.w_dev["B"][n], ref["g:" + n]
        exact = adam_fp64(p0.double(), g.double(), torch.zeros_like(p0).double(), torch.zeros_like(p0).double(), 1, PY["lr"])[0]
        q = torch.nn.Parameter(p0.clone())
        q.grad = g.clone()
        torch.optim.Adam([q], lr=PY["lr"], foreach=False).step()
        e_k, e_t = max(e_k, float((ref["w:" + n].double() - exact).abs().max())), max(e_t, float((q.detach().double() - exact).abs().max()))
        big = max(big, float(exact.abs().max()))
        assert float((T.w_dev["A"][n] - p0).abs().max()) >= POISON * float(np.spacing(np.float32(big)))
    within_bar(what + " stepped weights", e_k, e_t, big)


def compare_bits(what, got, ref):
    bad = [k for k in ref if not same_bits(got[k], ref[k])]
    assert not bad, "%s: %d of %d tensors differ from the default-stream step: %s" % (what, len(bad), len(ref), bad[:6])


def training_case(what, streams, monkeypatch, group, SB, B, parallel=False, two_streams=False):
    import test_gpu_grad_shapes as gs
    gs.set_leg("f16x2_default", monkeypatch)
    monkeypatch.setenv("PNYOLO_GROUP", group)
    for var in ("PNYOLO_SCENE_STREAMS", "PNYOLO_SPLIT_FLUSH", "PNYOLO_STASH_GB", "PNYOLO_PROJECTION"):
        monkeypatch.delenv(var, raising=False)
    T = Trainer(SB, B)
    if parallel:
        T.call = T.ren.bind_parallel(T.net, [0, 0])
    user, other = streams.s1, streams.s2

    def step():
        T.encode()
        T.render_and_step()
    # 1. the step on the default stream, against float64
    T.prepare("B")
    step()
    ref = T.collect()
    if not parallel:
        assert T.net._last_call_group == (group == "1")
        assert T.net.last_backward_precision() == "f16x2" and T.net.last_latent_grad_deterministic()
    check_training_reference(what, T, ref)
    # 2. poison: data set A, serially, on the user stream(s)
    T.prepare("A")
    with torch.cuda.stream(user):
        T.encode()
    if two_streams:
        other.wait_stream(user)
    with torch.cuda.stream(other if two_streams else user):
        T.render_and_step()
    T.collect()
    # 3. behind the spin
    T.prepare("B")

    def enqueue():
        with torch.cuda.stream(user):
            T.encode()
        if two_streams:
            other.wait_stream(user)        # the caller's own ordering: the documented use of two streams
        with torch.cuda.stream(other if two_streams else user):
            T.render_and_step()
    py_window(what, user, enqueue)
    compare_bits(what, T.collect(), ref)


@pytest.mark.parametrize("group", ["0", "1"])
def test_training_step_on_a_user_stream(group, streams, monkeypatch):
    """encode() of SB = 3 objects on a supplied latent that requires grad, NeRFRenderer in train mode with explicit draws, the
    loss behind _SlowIdentity, backward(), the project's Adam step (which refreshes the packed weights), all inside
    `with torch.cuda.stream(user)` behind the spin.  PNYOLO_GROUP=0: one scene and one side stream per object, forward and
    backward, the deferred weight-gradient flush behind their join; PNYOLO_GROUP=1: the grouped scene.  Rendered colours,
    parameter gradients, latent gradient and stepped weights bit-equal to the same step on the default stream, which is held
    to the float64 oracle (colours TOL, gradients RTOL, weights test_gpu_optim.py's rule)."""
    training_case("training_step[group=%s]" % group, streams, monkeypatch, group, SB=3, B=32)


def test_training_step_bind_parallel_on_a_user_stream(streams, monkeypatch):
    """The same through ren.bind_parallel(net, [0, 0]): two replicas on the device, each with half of the 128 rays of one
    object (a call of at least 64 rays per device splits), their latent-gradient shares summed by autograd.  The window
    assertion found a host synchronisation here: the wrapper brought its second replica up to date by copying EVERY tensor of the
    master's state_dict in place, code._freqs included, and the replica answered a changed tensor outside the MLPs and the trunk
    with a full re-upload (device-to-host copies and a pny_model_finalize, which waits for the device) on every training step:
    the host left the window after 83 ms.  With only the changed tensors copied it leaves after 6 ms."""
    training_case("training_step[bind_parallel]", streams, monkeypatch, "1", SB=1, B=128, parallel=True)


def test_encode_on_one_stream_render_on_another(streams, monkeypatch):
    """encode() on one user stream behind the spin, then -- after the caller's own wait_stream, the documented use -- render,
    backward and the optimizer step on another: bit-equal to the single-stream step."""
    training_case("training_step[two streams]", streams, monkeypatch, "0", SB=3, B=32, two_streams=True)


def test_no_grad_render_on_a_user_stream(streams, monkeypatch):
    """encode() and a no-grad render of SB = 3 objects (one scene and one side stream each, forked from the user stream) inside
    `with torch.cuda.stream(user)` behind the spin.  f16_range_policy = 'lazy': the default policy waits for the stream after
    a no-grad f16x2 call by design (model.guard_f16_range), which is a host synchronisation of the caller's choosing.  Coarse
    colours under TOL against float64; fine colours under TOL on all rays but at most one (an importance-sampling bin may
    flip: __graft_entry__.smoke's rule); everything bit-equal to the default-stream call."""
    import test_gpu_grad_shapes as gs
    gs.set_leg("f16x2_default", monkeypatch)
    monkeypatch.delenv("PNYOLO_SCENE_STREAMS", raising=False)
    SB, B = 3, 32
    T = Trainer(SB, B)
    T.net.f16_range_policy = "lazy"
    user = streams.s1

    def call():
        with torch.no_grad():
            T.encode()
            T.ren.draws = T.draws
            T.out = T.ren(T.net, T.rays, want_weights=True)

    def collect():
        torch.cuda.synchronize()
        return {p + "_" + k: v.clone() for p in ("coarse", "fine") for k, v in T.out[p].items()}
    T.prepare("B")
    call()
    ref = collect()
    o_b, o_a = py_oracle("B", SB, B), py_oracle("A", SB, B)
    e_c = metric("abs", ref["coarse_rgb"].cpu().numpy(), o_b["rgb_c"].numpy())
    over = int(((ref["fine_rgb"].cpu().double() - o_b["rgb_f"]).abs().amax(dim=-1) >= TOL).sum())
    print("STREAMS no_grad_render coarse rgb vs float64 %.3e (bar %.1e), fine rays over the bar: %d of %d" % (e_c, TOL, over, SB * B))
    assert e_c < TOL and over <= 1
    assert metric("abs", o_a["rgb_c"].numpy(), o_b["rgb_c"].numpy()) >= POISON * TOL
    assert metric("abs", o_a["rgb_f"].numpy(), o_b["rgb_f"].numpy()) >= POISON * TOL
    T.prepare("A")
    with torch.cuda.stream(user):
        call()
    collect()

    def enqueue():
        with torch.cuda.stream(user):
            call()
    T.prepare("B")
    py_window("no_grad_render", user, enqueue)
    compare_bits("no_grad_render", collect(), ref)


def test_zz_report(streams):
    """The figures of this module's run: the streams chosen, the spin, the largest host issue time inside a window."""
    if HOST_MS:
        worst = max(HOST_MS, key=HOST_MS.get)
        print("STREAMS report: %s; spin %d x SPIN_CYCLES = %d cycles; largest host issue time inside a window %.2f ms (%s) of %d windows"
              % (CHOSEN.get("streams"), SPIN, SPIN * SPIN_CYCLES, HOST_MS[worst], worst, len(HOST_MS)))
