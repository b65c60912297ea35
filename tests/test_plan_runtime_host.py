"""The plan runtime shared by the ResNet and Swin engines (models/_plan_engine.py), driven on the CPU with recording fakes:
the interpreter of the launch-list roles against the role table at the top of csrc/pfr_plan.hip, and the plan cache
(slots per forward pass in flight, eviction, rebuild after a tuning change).  No GPU, no shared library."""
import gc

import pytest

from pets_face_recognition_amd._hip import lib, PfrError
from pets_face_recognition_amd._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from pets_face_recognition_amd.models._plan_engine import Plan, PlanEngine, PlanTicket, run_ops


class FakeStream:
    def __init__(self, name, handle, trace):
        self.name, self.cuda_stream, self.trace = name, handle, trace

    def wait_event(self, e):
        self.trace.append(("wait", self.name, e.index))


class FakeEvent:
    def __init__(self, index, trace):
        self.index, self.trace = index, trace

    def record(self, stream):
        self.trace.append(("record", self.index, stream.name))


MAIN, SIDE_H = 0x1000, 0x2000    # raw stream handles the launches receive as their last argument


def _scene():
    trace = []

    def launch(name):
        def fn(*args):
            trace.append(("launch", name, args[:-1], {MAIN: "main", SIDE_H: "side"}[args[-1]]))
        fn.__name__ = name
        return fn

    # a main launch; fork / side launch / record (side op 1 -> events 2, 3); a hook-only wait; a hook stop; a main launch;
    # the final wait; the final hook stop
    ops = [(launch("a"), (1, 2.5)),
           (FORK, 1), (SIDE, (launch("s"), (3,))), (SREC, 1),
           (MWAIT, 1),
           (None, (128,)),
           (launch("b"), ()),
           (WAIT, 1),
           (None, (0,))]
    main = FakeStream("main", MAIN, trace)
    side = FakeStream("side", SIDE_H, trace)
    events = [FakeEvent(i, trace) for i in range(4)]

    def hook(off):
        trace.append(("hook", off))
    return ops, main, side, events, hook, trace


# csrc/pfr_plan.hip: 0 launch on the main stream | 1 launch on the side stream (main when the side stream is disabled) |
# 2 fork: record event ev on main, side waits for it | 3 record event ev on side | 4 main waits for event ev | 5 as 4, but only when
# the caller asked for hook stops (hook_stops 1; 2 = the hook synchronises with the side stream itself) | 6 hook stop.
# FORK k uses event 2k, SREC / WAIT / MWAIT k event 2k + 1 (_hip/cplan.py CPlan.compile).
A = ("launch", "a", (1, 2.5), "main")
B = ("launch", "b", (), "main")
FORK_JOIN = [("record", 2, "main"), ("wait", "side", 2), ("launch", "s", (3,), "side"), ("record", 3, "side")]
JOIN = ("wait", "main", 3)


def test_interpreter_side_stream_off():
    ops, main, side, events, hook, trace = _scene()
    run_ops(ops, main, None, [], None, False)
    assert trace == [A, ("launch", "s", (3,), "main"), B]
    del trace[:]
    run_ops(ops, main, None, [], hook, False)     # hook stops are served, the sync kinds stay no-ops
    assert trace == [A, ("launch", "s", (3,), "main"), ("hook", 128), B, ("hook", 0)]


def test_interpreter_side_stream_without_hook():
    ops, main, side, events, hook, trace = _scene()
    run_ops(ops, main, side, events, None, False)
    assert trace == [A] + FORK_JOIN + [B, JOIN]
    del trace[:]
    run_ops(ops, main, side, events, None, True)  # hook_syncs_side means nothing without a hook
    assert trace == [A] + FORK_JOIN + [B, JOIN]


def test_interpreter_side_stream_with_hook():
    ops, main, side, events, hook, trace = _scene()
    run_ops(ops, main, side, events, hook, False)
    assert trace == [A] + FORK_JOIN + [JOIN, ("hook", 128), B, JOIN, ("hook", 0)]


def test_interpreter_side_stream_with_hook_that_syncs_side():
    ops, main, side, events, hook, trace = _scene()
    run_ops(ops, main, side, events, hook, True)
    assert trace == [A] + FORK_JOIN + [("hook", 128), B, JOIN, ("hook", 0)]


# ------------------------------------------------------------------------------------------------ plan cache
class StubEngine(PlanEngine):
    def __init__(self):
        self._init_runtime()
        self.built = []

    def build_plan(self, *key):
        self.built.append(key)
        plan = Plan()
        plan.meta["n_fwd"] = 0
        return plan


@pytest.fixture
def epoch(monkeypatch):
    ep = [7]
    monkeypatch.setitem(vars(lib), "pfr_tuning_epoch", lambda: ep[0])
    return ep


SHAPE = (4, 32, 32, True)


def test_busy_shape_gets_another_slot_and_is_reusable_after_its_ticket_dies(epoch):
    eng = StubEngine()
    t1, t2 = PlanTicket(), PlanTicket()
    p1 = eng.acquire_plan(*SHAPE, ticket=t1)
    p2 = eng.acquire_plan(*SHAPE, ticket=t2)
    assert p1 is not p2 and eng.built == [SHAPE, SHAPE]
    assert eng.acquire_plan(*SHAPE, ticket=None) is p1         # no ticket (no backward will follow): slot 0 as it is
    del t1
    gc.collect()
    t3 = PlanTicket()
    assert eng.acquire_plan(*SHAPE, ticket=t3) is p1            # the autograd node died: its plan is free again
    p2.meta["owner"] = None                                     # what a backward pass does
    t4 = PlanTicket()
    assert eng.acquire_plan(*SHAPE, ticket=t4) is p2
    assert len(eng.built) == 2


def test_ninth_forward_pass_in_flight_raises(epoch):
    eng = StubEngine()
    tickets = [PlanTicket() for _ in range(9)]
    plans = [eng.acquire_plan(*SHAPE, ticket=t) for t in tickets[:8]]
    assert len({id(p) for p in plans}) == 8
    with pytest.raises(PfrError, match="more than 8 forward passes of one shape are waiting for their backward pass"):
        eng.acquire_plan(*SHAPE, ticket=tickets[8])


def test_eviction_takes_the_oldest_idle_plan_never_a_busy_one(epoch):
    eng = StubEngine()
    assert eng.max_plans == 8
    busy = PlanTicket()
    first = eng.acquire_plan(1, 32, 32, True, ticket=busy)
    idle = [eng.acquire_plan(n, 32, 32, True, ticket=None) for n in range(2, 9)]
    assert len(eng.plans) == 8
    ninth = eng.acquire_plan(9, 32, 32, True, ticket=None)
    assert len(eng.plans) == 8
    kept = list(eng.plans.values())
    assert first in kept and ninth in kept and idle[0] not in kept and all(p in kept for p in idle[1:])
    # every plan busy: nothing is evicted, the cache grows instead
    tickets = []
    for key in [k for k, p in eng.plans.items() if p is not first]:
        tickets.append(PlanTicket())
        eng.acquire_plan(*key, ticket=tickets[-1])
    assert len(eng.plans) == 8
    eng.acquire_plan(10, 32, 32, True, ticket=None)
    assert len(eng.plans) == 9 and first in eng.plans.values()


def test_tuning_epoch_change_drops_idle_plans_only(epoch):
    eng = StubEngine()
    busy = PlanTicket()
    held = eng.acquire_plan(1, 32, 32, True, ticket=busy)
    idle = eng.acquire_plan(2, 32, 32, True, ticket=None)
    assert eng.acquire_plan(2, 32, 32, True, ticket=None) is idle and len(eng.built) == 2    # same epoch: cached
    epoch[0] += 1
    rebuilt = eng.acquire_plan(2, 32, 32, True, ticket=None)
    assert rebuilt is not idle and len(eng.built) == 3
    assert held in eng.plans.values() and idle not in eng.plans.values()
    t = PlanTicket()
    assert eng.acquire_plan(1, 32, 32, True, ticket=t) is not held      # (still owned by `busy`: a second slot)
