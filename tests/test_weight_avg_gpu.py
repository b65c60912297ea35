"""Weight averaging on the device: the averaging optimizer steps (pfr_sgd_step_avg / pfr_adamw_step_avg) and the standalone lerp
(pfr_weight_avg) against the existing steps and an fp64 lerp; FusedSGD / FusedAdamW.attach_average against
torch.optim.swa_utils.AveragedModel; swap_averaged() through the engine; BatchNorm's cumulative moving average (momentum=None) and
utils.update_bn against torch on the CPU."""
import copy

import pytest
import torch
from torch.optim import swa_utils

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
WEIGHTS = (1.0, 0.5, 1.0 / 7.0, 1e-3)
SIZES = (1, 3, 63, 64, 65, 4099, 2 ** 20 + 3)


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _lerp_errors(got, a0, p, w):
    """(error of `got`, error of torch's own fp32 lerp on the CPU) against the lerp in fp64, max abs over the tensor"""
    a64, p64 = a0.double().cpu(), p.double().cpu()
    ref = a64 + (p64 - a64) * w
    t32 = a0.cpu().clone()
    torch._foreach_lerp_([t32], [p.cpu()], w)
    return (got.double().cpu() - ref).abs().max().item(), (t32.double() - ref).abs().max().item()


# Bound of every averaged buffer: 2 x the largest error torch's fp32 lerp shows against fp64 on the same inputs (the factor allows
# for FMA contraction).  Measured on an MI355X for pfr_weight_avg and pfr_sgd_step_avg: the ratio kernel error / torch error is 1.0 in
# every case of the sweep (the two fmaf forms round like torch's vectorised CPU lerp), 0 / 0 at weight 1 (both copy exactly); the sweep
# prints the ratio per size.
def _check_avg(got, a0, p, w, what):
    e, bound = _lerp_errors(got, a0, p, w)
    assert e <= 2 * bound, (what, e, bound)
    return e, bound


def _guarded(n, g, fill=None):
    t = torch.randn(n + GUARD, generator=g)
    if fill is not None:
        t[:n] = fill
    t[n:] = 12345.0
    return t.to(DEV)


@pytest.mark.parametrize("n", SIZES)
def test_standalone_weight_avg(n):
    from pets_face_recognition_amd._hip import ops
    g = torch.Generator().manual_seed(n)
    for off in (0, 1):                       # off 1: both views start one float past a 16-byte boundary
        for poff in (0, 1):                  # ... or only one of them (phases differ: the all-scalar path)
            for w in WEIGHTS:
                abuf, pbuf = _guarded(n + 1, g), torch.randn(n + 1, generator=g).to(DEV)
                a, p = abuf[off:off + n], pbuf[poff:poff + n]
                a0, before = a.clone(), abuf.clone()
                ops.weight_avg(a, p, w)
                _check_avg(a, a0, p, w, (n, off, poff, w))
                assert torch.equal(abuf[:off], before[:off]) and torch.equal(abuf[off + n:], before[off + n:])
                if w == 1.0:
                    assert torch.equal(a, p)


@pytest.mark.parametrize("n", SIZES)
def test_fused_steps_with_average_match_the_plain_steps_bit_for_bit(n):
    from pets_face_recognition_amd._hip import ops
    g = torch.Generator().manual_seed(100 + n)
    coef = torch.tensor([0.37], device=DEV)
    worst = 0.0
    for wi, w in enumerate(WEIGHTS):
        for mom in (0.0, 0.9):
            for wd in (0.0, 1e-4):
                for clip in (False, True):
                    for shadow_bf16 in (False, True):
                        p0, gr = torch.randn(n, generator=g).to(DEV), torch.randn(n, generator=g).to(DEV)
                        m0, v0 = torch.randn(n, generator=g).to(DEV), torch.rand(n, generator=g).to(DEV)
                        a0 = _guarded(n, g)
                        cc, cv = (coef, 0.5) if clip else (None, 0.0)
                        what = (n, w, mom, wd, clip, shadow_bf16)

                        def sh():
                            return torch.zeros(n, dtype=torch.bfloat16, device=DEV) if shadow_bf16 else None
                        # SGD
                        pr, mr, sr = p0.clone(), m0.clone(), sh()
                        if clip:
                            ops.sgd_step_clip(pr, gr, mr, sr, 0.05, mom, wd, cc, cv)
                        else:
                            ops.sgd_step(pr, gr, mr, sr, 0.05, mom, wd)
                        pa, ma, sa, av = p0.clone(), m0.clone(), sh(), a0.clone()
                        ops.sgd_step_avg(pa, gr, ma, sa, 0.05, mom, wd, cc, cv, av, w)
                        assert torch.equal(pa, pr) and torch.equal(ma, mr), what
                        assert sr is None or torch.equal(sa, sr), what
                        assert torch.equal(av[n:], a0[n:]), what
                        e, b = _check_avg(av[:n], a0[:n], pr, w, ("sgd",) + what)
                        worst = max(worst, e / b if b else 0.0)
                        # AdamW
                        pr, mr, vr, sr = p0.clone(), m0.clone(), v0.clone(), sh()
                        if clip:
                            ops.adamw_step_clip(pr, gr, mr, vr, sr, 1e-2, 0.9, 0.999, 1e-8, wd, 3, cc, cv)
                        else:
                            ops.adamw_step(pr, gr, mr, vr, sr, 1e-2, 0.9, 0.999, 1e-8, wd, 3)
                        pa, ma, va, sa, av = p0.clone(), m0.clone(), v0.clone(), sh(), a0.clone()
                        ops.adamw_step_avg(pa, gr, ma, va, sa, 1e-2, 0.9, 0.999, 1e-8, wd, 3, cc, cv, av, w)
                        assert torch.equal(pa, pr) and torch.equal(ma, mr) and torch.equal(va, vr), what
                        assert sr is None or torch.equal(sa, sr), what
                        assert torch.equal(av[n:], a0[n:]), what
                        e, b = _check_avg(av[:n], a0[:n], pr, w, ("adamw",) + what)
                        worst = max(worst, e / b if b else 0.0)
    print(f"n={n}: worst kernel / torch lerp error ratio {worst:.3f}")


# ------------------------------------------------------------------------------------------------ optimizer trajectories
def _small_resnet(dtype, momentum=0.1, seed=1, block="basic", layers=(1, 1, 1, 1)):
    from pets_face_recognition_amd.models.resnet import ResNet, BasicBlock, Bottleneck
    torch.manual_seed(seed)
    m = ResNet(BasicBlock if block == "basic" else Bottleneck, list(layers), compute_dtype=dtype)
    m.fc = torch.nn.Linear(m.fc.in_features, 64)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = momentum
    return m


def _groups(m):
    """the reference's three param groups (backbone, fc, head) with a Linear standing in for the margin head's weight"""
    p1 = [p for n, p in m.named_parameters() if "fc" not in n]
    p2 = [p for n, p in m.named_parameters() if "fc" in n]
    return [{"lr": 0.005, "params": p1}, {"lr": 0.01, "params": p2}]


def _make_opt(kind, m, head):
    from pets_face_recognition_amd.optim import FusedSGD, FusedAdamW
    groups = _groups(m) + [{"lr": 0.01, "params": [head], "weight_decay": 1e-4}]
    return FusedSGD(groups, 0.01, momentum=0.9) if kind == "sgd" else FusedAdamW(groups, 1e-3)


def _run(kind, avg, steps, batches, resume_at=None):
    """-> (live parameters after every step (CPU), final averages (CPU) or None, optimizer)"""
    m = _small_resnet(torch.float32).to(DEV).train()
    torch.manual_seed(2)
    head = torch.nn.Parameter(torch.randn(10, 64, device=DEV) * 0.05)
    opt = _make_opt(kind, m, head)
    if avg is not None:
        opt.attach_average(*avg)
    params = [p for g in opt.param_groups for p in g["params"]]
    live = []
    for i in range(steps):
        if resume_at is not None and i == resume_at:
            sd = copy.deepcopy(opt.state_dict())
            opt = _make_opt(kind, m, head)
            opt.load_state_dict(sd)
        opt.zero_grad()
        x, y = batches[i]
        loss = torch.nn.functional.cross_entropy(m(x) @ head.t(), y)
        loss.backward()
        opt.step()
        if avg is not None and avg[0] == "swa" and (i + 1) % 3 == 0:
            opt.update_average()
        live.append([p.detach().cpu().clone() for p in params])
    avgs = [opt.state[p]["avg"].detach().cpu().clone() for p in params] if avg is not None else None
    return live, avgs, opt


@pytest.fixture(scope="module")
def batches():
    g = torch.Generator().manual_seed(9)
    return [(torch.rand(4, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 10, (4,), generator=g).to(DEV)) for _ in range(15)]


@pytest.mark.parametrize("kind,avg", [("sgd", ("ema", 0.9)), ("adamw", ("ema", 0.9)), ("sgd", ("swa", None))])
def test_optimizer_average_follows_averaged_model(kind, avg, batches):
    steps = 12
    plain, _, _ = _run(kind, None, steps, batches)
    live, avgs, opt = _run(kind, avg, steps, batches)
    for a, b in zip(plain, live):                                 # the live parameters do not know about the average
        assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert opt.n_averaged == (steps if avg[0] == "ema" else steps // 3)
    # AveragedModel fed with the same live parameters: only the averaging is compared.  fp64 copy for the bound.
    holder = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in live[0]])
    fn = swa_utils.get_ema_multi_avg_fn(0.9) if avg[0] == "ema" else swa_utils.get_swa_multi_avg_fn()
    ref = swa_utils.AveragedModel(holder, multi_avg_fn=fn)
    a64, n_avg, single = None, 0, [0.0] * len(live[0])
    for i, ps in enumerate(live):
        if avg[0] == "swa" and (i + 1) % 3:
            continue
        with torch.no_grad():
            for h, t in zip(holder, ps):
                h.copy_(t)
        prev = [q.detach().clone() for q in ref.module.parameters()]
        ref.update_parameters(holder)
        w = 1.0 if n_avg == 0 else (1 - 0.9 if avg[0] == "ema" else 1.0 / (n_avg + 1))
        a64 = [t.double() for t in ps] if a64 is None else [a + (t.double() - a) * w for a, t in zip(a64, ps)]
        if n_avg:       # the error of this one fp32 lerp of torch's against the same lerp in fp64
            for k, (a0, t, q) in enumerate(zip(prev, ps, ref.module.parameters())):
                one = a0.double() + (t.double() - a0.double()) * w
                single[k] = max(single[k], (q.detach().double() - one).abs().max().item())
        n_avg += 1
    # bound: 2 x torch's largest single-lerp error (the kernel sweep's bound), scaled by the number of updates
    for got, r64, s1 in zip(avgs, a64, single):
        assert (got.double() - r64).abs().max().item() <= 2 * n_avg * s1
    # state_dict -> fresh optimizer -> load_state_dict -> 3 more steps == the uninterrupted run
    full_live, full_avgs, full_opt = _run(kind, avg, steps + 3, batches)
    res_live, res_avgs, res_opt = _run(kind, avg, steps + 3, batches, resume_at=steps)
    assert res_opt.n_averaged == full_opt.n_averaged
    assert all(torch.equal(x, y) for x, y in zip(full_live[-1], res_live[-1]))
    assert all(torch.equal(x, y) for x, y in zip(full_avgs, res_avgs))


def test_step_without_an_average_launches_what_it_did(batches, monkeypatch):
    from pets_face_recognition_amd._hip import ops
    calls = []
    for name in ("sgd_step", "sgd_step_clip", "sgd_step_avg", "weight_avg"):
        monkeypatch.setattr(ops, name, (lambda f, nm: lambda *a, **k: (calls.append(nm), f(*a, **k))[1])(getattr(ops, name), name))
    _run("sgd", None, 1, batches)
    assert calls and set(calls) == {"sgd_step"}
    calls.clear()
    _run("sgd", ("ema", 0.9), 1, batches)
    assert calls and set(calls) == {"sgd_step_avg"}
    calls.clear()
    _run("sgd", ("swa", None), 3, batches)
    assert set(calls) == {"sgd_step", "weight_avg"} and calls.count("weight_avg") == len([c for c in calls if c == "sgd_step"]) // 3


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_swap_averaged_reaches_the_engine(dtype, batches):
    from pets_face_recognition_amd.optim import FusedSGD
    m = _small_resnet(dtype).to(DEV).train()
    opt = FusedSGD(_groups(m), 0.01, momentum=0.9)
    opt.attach_average("ema", 0.5)
    for i in range(3):
        opt.zero_grad()
        m(batches[i][0]).square().mean().backward()
        opt.step()
    x = batches[3][0]
    m.eval()
    with torch.no_grad():
        before = m(x).clone()
        live_sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        with opt.swap_averaged():
            inside = m(x).clone()
            avg_sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        after = m(x).clone()
    assert torch.equal(after, before)
    assert all(torch.equal(v.cpu(), live_sd[k]) for k, v in m.state_dict().items())
    assert not torch.equal(avg_sd["conv1.weight"], live_sd["conv1.weight"])
    assert all(torch.equal(avg_sd[k], live_sd[k]) for k in live_sd if "running_" in k)
    m2 = _small_resnet(dtype, seed=5)
    m2.load_state_dict(avg_sd)
    m2 = m2.to(DEV).eval()
    with torch.no_grad():
        want = m2(x)
    assert torch.equal(inside, want)
    assert not torch.equal(inside, before)


# ------------------------------------------------------------------------------------------------ BatchNorm momentum=None
def _op_names(plan):
    from pets_face_recognition_amd._hip.cplan import SIDE
    names = []
    for fn, args in plan.meta["fwd"]:
        if callable(fn):
            names.append(fn.__name__)
        elif fn == SIDE:
            names.append(args[0].__name__)
    return names


def _bn_state(m):
    return {k: v.detach().cpu().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k}


def _assert_bn_close(got, want, tol):
    assert list(got) == list(want)
    for k in want:
        if "num_batches" in k:
            assert int(got[k]) == int(want[k]), k
        else:
            assert rel(got[k], want[k]) < tol, (k, rel(got[k], want[k]))


@pytest.fixture(scope="module")
def bn_batches():
    g = torch.Generator().manual_seed(21)
    return [torch.rand(8, 3, 32, 32, generator=g) for _ in range(5)]


TOL = 5e-3      # the fp32 running-statistics tolerance of tests/test_model_gpu.py (5 x its 1e-3 embedding tolerance)


def test_bn_cumulative_moving_average(bn_batches):
    cpu = _small_resnet(torch.float32, momentum=None).train()
    m = copy.deepcopy(cpu).to(DEV).train()
    with torch.no_grad():
        for x in bn_batches:
            cpu(x)
            m(x.to(DEV))
    _assert_bn_close(_bn_state(m), _bn_state(cpu), TOL)
    assert int(m.state_dict()["bn1.num_batches_tracked"]) == 5
    # with backward too (the training plan)
    m(bn_batches[0].to(DEV)).sum().backward()
    cpu(bn_batches[0]).sum().backward()
    _assert_bn_close(_bn_state(m), _bn_state(cpu), TOL)


def test_float_momentum_plans_are_what_they_were(bn_batches):
    x = bn_batches[0].to(DEV)
    fresh = _small_resnet(torch.float32).to(DEV).train()         # never saw momentum=None
    twin = _small_resnet(torch.float32).to(DEV).train()
    with torch.no_grad():
        fresh(x)
        twin(x)                                                     # the engine adopts the float momenta
        float_plan = twin.hip_engine()._last_plan
        for mod in twin.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.momentum = None
        twin(x)
        e = twin.hip_engine()
        cumulative_plan = e._last_plan
        for mod in twin.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.momentum = 0.1
        twin.load_state_dict(copy.deepcopy(_small_resnet(torch.float32).state_dict()))
        twin(x)
    assert cumulative_plan is not float_plan                      # no plan of another momentum is reused, either way
    assert e._last_plan is float_plan
    assert e._plan_tag() == () and e.cma is not None
    assert _op_names(e._last_plan) == _op_names(fresh.hip_engine()._last_plan)
    assert "pfr_weight_avg" not in _op_names(e._last_plan)
    _assert_bn_close(_bn_state(twin), _bn_state(fresh), 1e-6)
    # a mixed model: only the momentum=None BatchNorms average cumulatively
    cpu = _small_resnet(torch.float32).train()
    cpu.layer2[0].bn1.momentum = None
    cpu.bn1.momentum = None
    mixed = copy.deepcopy(cpu).to(DEV).train()
    with torch.no_grad():
        for xb in bn_batches[:3]:
            cpu(xb)
            mixed(xb.to(DEV))
    _assert_bn_close(_bn_state(mixed), _bn_state(cpu), TOL)


def test_update_bn_matches_swa_utils(bn_batches):
    from pets_face_recognition_amd.utils import update_bn
    cpu = _small_resnet(torch.float32).train()
    with torch.no_grad():
        cpu(bn_batches[0])                                         # statistics that the reset must forget
    m = copy.deepcopy(cpu).to(DEV).eval()
    cpu.eval()
    swa_utils.update_bn(bn_batches, cpu)
    update_bn(bn_batches, m, device=DEV)
    assert not m.training and all(mod.momentum == 0.1 for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d))
    _assert_bn_close(_bn_state(m), _bn_state(cpu), TOL)
    # a model without BatchNorm returns at once (the loader is not touched)
    update_bn(iter(lambda: pytest.fail("loader read"), None), torch.nn.Linear(3, 3))


def test_bn_cumulative_average_at_the_streaming_finalize_sites():
    """bf16 bottlenecks: the Gram / streaming statistics finalize sites take the momentum too.  At 16 x 3 x 64 x 64 the engine
    selects none of them (layer1 has 4096 rows; pfr_conv1x1_tail_mtile and pfr_conv2d_dgrad_bn_parts answer 0 below 8192);
    32 x 3 x 64 x 64 is the smallest batch of 64 x 64 images that does."""
    g = torch.Generator().manual_seed(4)
    xs = [torch.rand(32, 3, 64, 64, generator=g) for _ in range(3)]
    cpu = _small_resnet(torch.float32, momentum=None, block="bottleneck", layers=(2, 1, 1, 1)).train()
    m = copy.deepcopy(cpu)
    m.compute_dtype = torch.bfloat16
    m = m.to(DEV).train()
    for x in xs:                      # under autograd: the BN-input-free forms belong to the training plan
        cpu(x)
        m(x.to(DEV))
    names = _op_names(m.hip_engine()._last_plan)
    print("finalize sites:", {k: names.count(k) for k in set(names) if "gram" in k or "tail" in k or "stats" in k or "finalize" in k})
    assert "pfr_bn_finalize_from_gram" in names or "pfr_conv1x1_stats" in names or any("bn_tail" in k for k in names)
    got, want = _bn_state(m), _bn_state(cpu)
    # bf16 activations: the bf16 tolerance of tests/test_model_gpu.py's running statistics (5 x 4e-2)
    _assert_bn_close(got, want, 0.2)
