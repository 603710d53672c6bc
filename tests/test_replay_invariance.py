"""GPU: every launching entry point of the C ABI run as production runs it -- recorded into a glsdet_plan whose host
arguments are then destroyed, replayed eagerly and from a captured hipGraph into the same buffers with other data, on a
workspace that keeps what the previous replay left -- and held bit for bit to what the same call gives when it launches
at once on freshly dirtied buffers.  Where the family has a bit-exact reference (tests/*_reference.py) the immediate
result is held to it first, so the replays answer to a reference and not only to the kernel itself.

Cases, data sets and the protocol of a case: tests/replay_cases.py.  One process, one stream at a time."""
import gc
import math

import pytest
import torch                            # before the library is loaded: both must share one HIP runtime

from tests import replay_cases as RC

pytestmark = pytest.mark.gpu
_state = {}


def _keys():
    import __graft_entry__ as g
    g.build()
    return [c.key for c in RC.cases()]


KEYS = _keys()


@pytest.fixture(scope="module")
def lib():
    from glsdet_amd import _lib
    return _lib.load()


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a failed comparison lets the module go on; a device error ends the session: nothing more is started on that GPU"""
    yield
    try:
        torch.cuda.synchronize()
    except Exception as e:                                           # noqa: BLE001
        pytest.exit("device error, no further GPU work is started: %s" % e, returncode=3)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _prepared(lib, key):
    """the case on device buffers with ref[k] = the outputs of the call made outside a recording, on dirtied outputs and workspaces"""
    if key not in _state:
        c = [q for q in RC.cases() if q.key == key][0].bind_device()
        ref = []
        for k in range(c.n_sets):
            c.dirty()
            c.load(k)
            _sync()
            c.record(lib, _stream())
            ref.append(c.outputs())
            c.destroy_host_args()
            assert c.in_place or c.inputs_changed(k) == [], (key, k, c.inputs_changed(k))
        _state[key] = (c, ref)
    return _state[key]


def _order(c):
    last = c.n_sets - 1
    return [last] + list(range(last - 1, -1, -1)) + [last]           # last, ..., 0, last


def _recorded(lib, cases):
    """one plan of the cases, recorded with set 0 loaded; every host argument destroyed and collected"""
    from glsdet_amd.engine import Plan
    plan = Plan(lib)
    for c in cases:
        c.load(0)
    _sync()
    with plan:
        for c in cases:
            c.record(lib, _stream())
    assert plan.num_ops >= len(cases)
    for c in cases:
        c.destroy_host_args()
    gc.collect()
    return plan


def _replay(cases, refs, run, what):
    """for k in (last, ..., 0, last): dirty the outputs (the workspace keeps what the previous replay left), load(k), run"""
    bad = []
    for step, pick in enumerate(_order(max(cases, key=lambda c: c.n_sets))):
        ks = [min(pick, c.n_sets - 1) for c in cases]
        for c, k in zip(cases, ks):
            c.dirty(ws=False)
            c.load(k)
        _sync()
        run()
        _sync()
        for c, k, ref in zip(cases, ks, refs):
            bad += ["%s, %s step %d (set %d): %s" % (c.key, what, step, k, d) for d in RC.differing(c.outputs(), ref[k])]
            if not c.in_place:
                bad += ["%s, %s step %d (set %d): input %s was written" % (c.key, what, step, k, nm) for nm in c.inputs_changed(k)]
    return bad


def _graph(plan):
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        plan.capture(st)
    st.synchronize()

    def launch():
        with torch.cuda.stream(st):
            plan.launch(st)
        st.synchronize()
    return launch


@pytest.mark.parametrize("key", KEYS)
def test_immediate_launch_equals_the_reference_and_differs_between_sets(lib, key):
    c, ref = _prepared(lib, key)
    if c.has_want:
        for k in range(c.n_sets):
            assert c.check_want(k, ref[k]) == [], (key, k)
    # the data sets must be told apart by the outputs, or a value frozen at record time would pass
    same = [k for k in range(1, c.n_sets) if not RC.differing(ref[k], ref[0])]
    assert not same, "%s: data sets %s give the outputs of set 0" % (key, same)


@pytest.mark.parametrize("key", KEYS)
def test_eager_replay_of_the_recorded_op(lib, key):
    c, ref = _prepared(lib, key)
    plan = _recorded(lib, [c])
    bad = _replay([c], [ref], lambda: plan.run(), "plan_run")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", KEYS)
def test_graph_replay_of_the_recorded_op(lib, key):
    c, ref = _prepared(lib, key)
    plan = _recorded(lib, [c])
    launch = _graph(plan)
    bad = _replay([c], [ref], launch, "plan_launch")
    c.dirty(ws=False)                                                # the last set once more
    c.load(_order(c)[-1])                                            # (an in-place op consumed it)
    _sync()
    launch()
    bad += RC.differing(c.outputs(), ref[_order(c)[-1]])
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("key", KEYS)
def test_timed_run_computes_what_plan_run_does(lib, key):
    c, ref = _prepared(lib, key)
    plan = _recorded(lib, [c])
    c.dirty(ws=False)
    c.load(0)
    _sync()
    ms = plan.run_timed()
    _sync()
    assert RC.differing(c.outputs(), ref[0]) == []
    assert len(ms) == plan.num_ops and all(math.isfinite(v) and v >= 0 for v in ms), ms


def test_one_plan_of_every_case_eagerly_and_from_a_graph(lib):
    """every case of the registry, second shapes included, in one plan: state shared between two ops of a kind (a launch
    attribute cached in a static for the first shape, a shared scratch buffer) shows here"""
    pairs = [_prepared(lib, key) for key in KEYS]
    cases, refs = [p[0] for p in pairs], [p[1] for p in pairs]
    plan = _recorded(lib, cases)
    bad = _replay(cases, refs, lambda: plan.run(), "plan_run")
    bad += _replay(cases, refs, _graph(plan), "plan_launch")
    assert not bad, "\n".join(bad[:40])
