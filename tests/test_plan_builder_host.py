"""PlanBuilder (models/_plan_engine.py), the build-time half of the plan runtime that the Swin, ConvNeXt, ViT, MobileNetV2 and
EfficientNet engines share: side-stream fork sharing, the backward buffer pool and the waits it emits, the symbolic weight-gradient
entry and the split-K workspace, grad-ready marks and the deferred column sums.  Driven on the CPU with CPU tensors and recording
fakes for the library functions the builder names or queries.  No GPU, no shared library."""
import struct

import pytest
import torch

from pets_face_recognition_amd._hip import lib
from pets_face_recognition_amd._hip.cplan import SIDE, FORK, SREC, WAIT, MWAIT
from pets_face_recognition_amd.models._plan_engine import Plan, PlanBuilder, PlanEngine

T = torch.bfloat16
DID = 1


def launch(name):
    def fn(*args):
        raise AssertionError(f"{name} launched while a plan was built")
    fn.__name__ = name
    return fn


MAIN_OP = (launch("main_op"), (1, 2))
COLSUM, COLSUM_PARTIAL, COLSUM_FINAL, WGRAD = (launch(n) for n in ("pfr_colsum", "pfr_colsum_partial", "pfr_colsum_final_batch",
                                                                    "pfr_conv2d_wgrad"))


@pytest.fixture
def fake_lib(monkeypatch):
    """queries answered from a table the test fills in; launches that only ever end up in a list"""
    q = {"splits": lambda M, Co, KK: 1, "colsum_parts": lambda d, rows, C: 0}
    monkeypatch.setitem(vars(lib), "pfr_conv2d_wgrad_splits", lambda *a: q["splits"](*a))
    monkeypatch.setitem(vars(lib), "pfr_colsum_parts", lambda *a: q["colsum_parts"](*a))
    monkeypatch.setitem(vars(lib), "pfr_colsum_ws_floats", lambda rows, C: 4 * C)
    for fn in (COLSUM, COLSUM_PARTIAL, COLSUM_FINAL, WGRAD):
        monkeypatch.setitem(vars(lib), fn.__name__, fn)
    return q


def builder(pool_depth=48):
    return PlanBuilder(Plan(), T, torch.device("cpu"), DID, pool_depth)


def side_op(name="side_op", *args):
    return (SIDE, (launch(name), args))


# ------------------------------------------------------------------------------------------------ fork sharing
def test_side_ops_without_a_main_launch_between_them_share_one_fork():
    pb = builder()
    op1, op2 = side_op("s1"), side_op("s2")
    pb.side(op1)
    pb.side(op2)
    assert pb.bwd == [(FORK, 0), op1, op2, (SREC, 0)]
    assert pb.nside == 1 and pb.fwd == []


def test_a_main_launch_between_side_ops_starts_a_second_fork():
    pb = builder()
    op1, op2 = side_op("s1"), side_op("s2")
    pb.side(op1)
    pb.bwd.append(MAIN_OP)
    pb.side(op2)
    assert pb.bwd == [(FORK, 0), op1, (SREC, 0), MAIN_OP, (FORK, 1), op2, (SREC, 1)]
    assert pb.nside == 2


# ------------------------------------------------------------------------------------------------ pool reuse and waits
def test_buffer_without_a_side_reader_is_handed_out_again_without_a_wait():
    pb = builder()
    a = pb.G((4, 8))
    assert a.dtype == T and tuple(a.shape) == (4, 8)
    pb.bwd.append(MAIN_OP)
    pb.release(a)
    assert pb.G((4, 8)) is a
    assert pb.bwd == [MAIN_OP]


def test_buffer_a_side_op_reads_is_left_alone_while_the_class_may_grow():
    pb = builder()
    a = pb.G((4, 8))
    pb.side(side_op("s0"), a)          # side op 0 reads a
    pb.bwd.append(MAIN_OP)
    pb.side(side_op("s1"), a)          # side op 1 reads a too
    pb.release(a)
    n = len(pb.bwd)
    b = pb.G((4, 8))
    assert b is not a and b.data_ptr() != a.data_ptr()
    assert pb.bwd[n:] == []            # a fresh allocation: nothing to wait for


def test_exhausted_class_hands_out_the_oldest_after_one_wait_for_its_later_reader():
    pb = builder(pool_depth=2)
    a, b = pb.G((4, 8)), pb.G((4, 8))      # the class has its two allocations
    pb.side(side_op("s0"), a)
    pb.bwd.append(MAIN_OP)
    pb.side(side_op("s1"), a, b)
    pb.bwd.append(MAIN_OP)
    pb.side(side_op("s2"), b)
    pb.release(a)                           # read by side ops 0 and 1
    pb.release(b)                           # read by side ops 1 and 2
    n = len(pb.bwd)
    got = pb.G((4, 8))
    assert got is a
    assert pb.bwd[n:] == [(WAIT, 1)]
    got2 = pb.G((4, 8))
    assert got2 is b
    assert pb.bwd[n:] == [(WAIT, 1), (WAIT, 2)]


def test_read_through_a_view_into_the_middle_of_a_buffer_counts():
    pb = builder(pool_depth=1)
    a = pb.G((4, 8))
    pb.side(side_op("s0"), a[2])            # a view that starts 32 bytes into the buffer
    assert a[2].data_ptr() != a.data_ptr()
    pb.release(a)
    n = len(pb.bwd)
    assert pb.G((4, 8)) is a
    assert pb.bwd[n:] == [(WAIT, 0)]


def test_another_shape_or_dtype_is_another_class():
    pb = builder(pool_depth=1)
    a = pb.G((4, 8))
    pb.release(a)
    assert pb.G((8, 4)) is not a
    f = pb.G((4, 8), torch.float32)
    assert f is not a and f.dtype == torch.float32
    assert pb.G((4, 8)) is a
    assert pb.bwd == []


# ------------------------------------------------------------------------------------------------ wgrad
class StubEngine(PlanEngine):
    def __init__(self):
        self._init_runtime()


def test_wgrad_is_symbolic_until_resolve_and_sizes_the_workspace(fake_lib):
    fake_lib["splits"] = lambda M, Co, KK: {(2 * 3 * 3, 16, 9 * 8): 3, (2 * 1 * 1, 32, 8): 5}[(M, Co, KK)]
    pb = builder()
    x, dy, out = pb.A((2, 6, 6, 8)), pb.A((2, 3, 3, 16)), pb.A((16 * 9 * 8,), torch.float32)
    pb.wgrad(x, (2, 6, 6, 8), dy, (2, 3, 3, 16), 3, 2, 1, out)
    fn, args = pb.bwd[1]
    assert pb.bwd[0] == (FORK, 0) and pb.bwd[2] == (SREC, 0)
    assert fn == "wgrad" and args[3] is None
    assert args == (x.data_ptr(), dy.data_ptr(), out.data_ptr(), None, DID, 2, 6, 6, 8, 16, 3, 3, 2, 1, 3, 3, 16, 0, 0, 0, 1.0, 0)
    assert pb.ws_need == 3 * 16 * 9 * 8
    x2, dy2 = pb.A((2, 1, 1, 8)), pb.A((2, 1, 1, 32))
    pb.wgrad(x2, (2, 1, 1, 8), dy2, (2, 1, 1, 32), 1, 1, 0, out)
    assert pb.ws_need == max(3 * 16 * 9 * 8, 5 * 32 * 8)
    # the side op reads dy: releasing dy makes it pending on that op
    pb.release(dy)
    assert pb.pending == {dy.data_ptr(): 0}

    eng = StubEngine()
    pb.plan.meta["n_fwd"] = len(pb.fwd)
    plan = pb.finish(eng)
    assert plan is pb.plan and plan.ops == pb.fwd + pb.bwd and plan.meta["n_side"] == 1
    assert eng.ws.dtype == torch.float32 and eng.ws.numel() == pb.ws_need
    eng.resolve(plan)
    kind, (rfn, rargs) = plan.meta["bwd"][1]
    assert kind == SIDE and rfn is lib.pfr_conv2d_wgrad
    assert rargs[3] == eng.ws.data_ptr() and rargs[-1] == 0
    assert rargs[:3] + rargs[4:-1] == args[:3] + args[4:-1]

    # a later, smaller plan leaves the engine's workspace alone
    ws = eng.ws
    small = builder()
    fake_lib["splits"] = lambda M, Co, KK: 1
    small.wgrad(x2, (2, 1, 1, 8), dy2, (2, 1, 1, 32), 1, 1, 0, out)
    small.finish(eng)
    assert eng.ws is ws


# ------------------------------------------------------------------------------------------------ mark, column sums
def test_mark_without_a_side_op_is_the_hook_stop_alone():
    pb = builder()
    pb.mark(128)
    pb.mark(0, last=True)
    assert pb.bwd == [(None, (128,)), (None, (0,))]


def test_mark_waits_for_the_last_side_op():
    pb = builder()
    op1, op2 = side_op("s1"), side_op("s2")
    pb.side(op1)
    pb.bwd.append(MAIN_OP)
    pb.side(op2)
    n = len(pb.bwd)
    pb.mark(256)
    assert pb.bwd[n:] == [(MWAIT, 1), (None, (256,))]
    n = len(pb.bwd)
    pb.mark(0, last=True)
    assert pb.bwd[n:] == [(WAIT, 1), (None, (0,))]


def test_mark_flushes_pending_column_sums_as_one_side_op_before_the_wait(fake_lib):
    pb = builder()
    w1, w2, w3 = (pb.A((6, c), torch.float32) for c in (8, 24, 16))
    o1, o2, o3 = (pb.A((c,), torch.float32) for c in (8, 24, 16))
    pb.pend_cs.append((w1, o1, 6, 8, 0, 0))
    pb.pend_cs.append((w2, o2, 3, 24, 64, 150))
    pb.pend_cs.append((w3, o3, 6, 16, 0, 0))
    pb.bwd.append(MAIN_OP)
    nbuf = len(pb.plan.bufs)
    pb.mark(512)
    assert pb.pend_cs == []
    assert pb.bwd[0] == MAIN_OP and pb.bwd[1] == (FORK, 0) and pb.bwd[3:] == [(SREC, 0), (MWAIT, 0), (None, (512,))]
    kind, (fn, (tab_ptr, count, width)) = pb.bwd[2]
    assert kind == SIDE and fn is lib.pfr_colsum_final_batch and count == 3 and width == 24
    tab = pb.plan.bufs[nbuf]                      # the table is kept alive by the plan
    assert tab.data_ptr() == tab_ptr and tab.dtype == torch.uint8
    recs = list(struct.iter_unpack("<QQiiiiii", bytes(tab.tolist())))
    assert recs == [(w1.data_ptr(), o1.data_ptr(), 6, 8, 0, 0, 0, 0),
                    (w2.data_ptr(), o2.data_ptr(), 3, 24, 0, 64, 150, 0),
                    (w3.data_ptr(), o3.data_ptr(), 6, 16, 0, 0, 0, 0)]
    # nothing pending: the next mark adds no flush
    n = len(pb.bwd)
    pb.mark(0, last=True)
    assert pb.bwd[n:] == [(WAIT, 0), (None, (0,))]


def test_colsum_of_a_few_rows_is_one_side_op_and_defers_nothing(fake_lib):
    fake_lib["colsum_parts"] = lambda d, rows, C: 0
    pb = builder()
    x, out = pb.A((5, 16)), pb.A((16,), torch.float32)
    pb.colsum(x, 5, 16, out)
    assert pb.bwd == [(FORK, 0), (SIDE, (lib.pfr_colsum, (x.data_ptr(), DID, 5, 16, out.data_ptr(), 0, 0))), (SREC, 0)]
    assert pb.pend_cs == []
    pb.release(x)                                 # the side op reads x
    assert pb.pending == {x.data_ptr(): 0}


def test_colsum_of_many_rows_runs_the_partials_now_and_defers_the_merge(fake_lib):
    fake_lib["colsum_parts"] = lambda d, rows, C: 7
    pb = builder()
    x, out = pb.A((500, 16), torch.float32), pb.A((16,), torch.float32)
    pb.colsum(x, 500, 16, out, 0)                 # its own dtype id, as the position-table sums of Swin
    (kind, (fn, args)) = pb.bwd[1]
    assert kind == SIDE and fn is lib.pfr_colsum_partial and args[:4] == (x.data_ptr(), 0, 500, 16)
    (ws, o, n, C, mt, rows), = pb.pend_cs
    assert ws.data_ptr() == args[4] and ws.numel() == 4 * 16 and ws.dtype == torch.float32
    assert (o.data_ptr(), n, C, mt, rows) == (out.data_ptr(), 7, 16, 0, 0)
