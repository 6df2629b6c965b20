"""CPU tests of the optimiser stage (include/tpspp_train_opt.h, tps_pp_amd/optim.py, the runner methods of
EncodeDecodeRecognizer): the header, the binding table and the shared object agree and stay out of the other three headers'
lists; argument errors come back as -22 with a message before anything is launched; the chunk map covers every element
once; build_optimizer restates mmcv's paramwise rule; a state_dict moves to torch.optim.Adam and back; _parse_losses; and
torch.optim's own rounding error on the inputs of tests/test_gpu_optim.py stays under the caps written there."""
import ctypes
import math
import os

import pytest
import torch

import test_gpu_optim as TG
from tps_pp_amd import EncodeDecodeRecognizer, _lib, build, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "tpspp_train_opt.h")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


def test_header_names_what_it_replaces():
    text = open(HEADER).read()
    assert "replaces:" in text
    for ref in ("torch.optim.Adam", "AdamW", "clip_grad_norm_", "OptimizerHook", "fused"):
        assert ref in text, ref


def test_argument_errors_are_codes_with_messages_and_launch_nothing(lib):
    """Every call names host memory (or nothing) as its operands: a launch would fail loudly, a -22 launches none."""
    keep = (ctypes.c_float * 64)()
    p = ctypes.cast(keep, ctypes.c_void_p).value
    err = lib.tpspp_last_error

    def adam(table=p, scalars=p, nt=1, cmap=p, nc=1, chunk=4096, threads=256, b1=0.9, b2=0.999, eps=1e-8, mode=0):
        return lib.tpspp_mt_adam(table, scalars, nt, cmap, nc, chunk, threads, b1, b2, eps, mode, None, None)

    def sumsq(table=p, nt=1, cmap=p, nc=1, chunk=4096, threads=256, partials=p, floats=1):
        return lib.tpspp_mt_sumsq(table, nt, cmap, nc, chunk, threads, partials, floats, None)

    def zero(table=p, nt=1, cmap=p, nc=1, chunk=4096, threads=256):
        return lib.tpspp_mt_zero(table, nt, cmap, nc, chunk, threads, None)

    for call in (adam, sumsq, zero):
        assert call(table=None) == -22 and b"null pointer" in err(), call
        assert call(cmap=None) == -22 and b"null pointer" in err(), call
        for bad in (0, -1):
            assert call(nt=bad) == -22 and b"must be positive" in err(), (call, bad)
            assert call(nc=bad) == -22 and b"must be positive" in err(), (call, bad)
        for bad in (0, -4, 4095, 6, (1 << 20) + 4):
            assert call(chunk=bad) == -22 and b"multiple of 4" in err(), (call, bad)
        for bad in (0, 32, 96, 2048):
            assert call(threads=bad) == -22 and b"threads" in err(), (call, bad)
    assert adam(scalars=None) == -22 and b"null pointer" in err()
    for bad in (-1, 2, 7):
        assert adam(mode=bad) == -22 and b"mode" in err(), bad
    for kw in (dict(b1=1.0), dict(b2=-0.1), dict(b1=float("nan"))):
        assert adam(**kw) == -22 and b"betas" in err(), kw
    for bad in (-1e-8, float("inf"), float("nan")):
        assert adam(eps=bad) == -22 and b"eps" in err(), bad
    assert sumsq(partials=None) == -22 and b"null pointer" in err()
    assert sumsq(nc=8, floats=7) == -22 and b"workspace" in err()
    assert lib.tpspp_mt_norm_finish(None, 1, 1.0, p, None) == -22 and b"null pointer" in err()
    assert lib.tpspp_mt_norm_finish(p, 1, 1.0, None, None) == -22 and b"null pointer" in err()
    assert lib.tpspp_mt_norm_finish(p, 0, 1.0, p, None) == -22 and b"must be positive" in err()
    for bad in (0.0, -1.0, float("nan")):
        assert lib.tpspp_mt_norm_finish(p, 1, bad, p, None) == -22 and b"max_norm" in err(), bad
    del keep


@pytest.mark.parametrize("chunk", [4, 8, 64, optim.CHUNK])
def test_chunk_map_covers_every_element_exactly_once_in_order(chunk):
    sizes = [1, 2, 3, chunk - 1, chunk, chunk + 1, 3 * chunk + 5, 0, 1]
    rows = optim.build_chunk_map(sizes, chunk)
    assert rows == sorted(rows)
    seen = [[] for _ in sizes]
    for ti, first in rows:
        assert first % chunk == 0 and 0 <= first < sizes[ti]
        seen[ti].extend(range(first, min(first + chunk, sizes[ti])))
    assert all(s == list(range(n)) for s, n in zip(seen, sizes))
    assert len(rows) == sum(-(-n // chunk) for n in sizes)
    assert optim.build_chunk_map([], chunk) == [] and optim.build_chunk_map([0, 0], chunk) == []
    for bad in (0, -4, 6, chunk + 1):
        with pytest.raises(ValueError, match="multiple of 4"):
            optim.build_chunk_map(sizes, bad)


def test_empty_parameter_lists_and_absent_gradients_launch_nothing():
    p = torch.nn.Parameter(torch.ones(3))
    opt = optim.Adam([p], lr=1e-3)
    assert opt.step() is None and len(opt.state) == 0 and opt.table_builds == 0      # no gradient: nothing to do, even on CPU
    opt.zero_grad()
    opt.zero_grad(set_to_none=False)
    p.grad = torch.ones(3)
    with pytest.raises(_lib.TpsppError, match=r"parameter 0 of group 0 \(3,\) is on cpu.*no CPU fallback"):
        opt.step()
    with pytest.raises(_lib.TpsppError, match="no CPU fallback"):
        opt.zero_grad(set_to_none=False)
    opt.zero_grad()
    assert p.grad is None
    for bad in (dict(amsgrad=True), dict(grad_clip=dict(max_norm=1.0, norm_type=1)),
                dict(grad_clip=dict(max_norm=1.0, norm_type="inf"))):
        with pytest.raises(NotImplementedError):
            optim.Adam([p], **bad)
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.9)), dict(eps=-1.0), dict(weight_decay=-1.0), dict(chunk=6),
                dict(threads=100), dict(grad_clip=dict(max_norm=0.0)), dict(grad_clip=dict(norm_type=2)),
                dict(grad_clip=dict(max_norm=1.0, error_if_nonfinite=True))):
        with pytest.raises(ValueError):
            optim.Adam([p], **bad)
    assert optim.AdamW([p]).defaults["weight_decay"] == 1e-2 and optim.Adam([p]).defaults["weight_decay"] == 0.0


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = torch.nn.Sequential(torch.nn.Conv2d(1, 2, 1), torch.nn.BatchNorm2d(2))
        self.encoder = torch.nn.Linear(2, 2)
        self.decoder = torch.nn.Linear(2, 2)
        self.decoder.bias.requires_grad_(False)


def test_build_optimizer_groups_as_mmcv_does():
    net = _Net()
    names = [n for n, _ in net.named_parameters()]
    plain = optim.build_optimizer(net, dict(type="Adam", lr=1e-4))
    assert isinstance(plain, optim.Adam) and len(plain.param_groups) == 1
    assert plain.param_groups[0]["lr"] == 1e-4 and plain.param_groups[0]["params"] == list(net.parameters())
    assert plain.max_norm is None and plain.param_names[id(net.encoder.weight)] == "encoder.weight"
    cfg = dict(type="AdamW", lr=1e-3, betas=(0.9, 0.99), eps=1e-6, weight_decay=0.1,
               paramwise_cfg=dict(custom_keys={"backbone": dict(lr_mult=0.1), "backbone.1": dict(lr_mult=0.0, decay_mult=0.0),
                                               "bias": dict(decay_mult=0.5), "encoder": dict(lr_mult=2.0, decay_mult=3.0)}))
    keep = dict(cfg, paramwise_cfg=dict(cfg["paramwise_cfg"]))
    opt = optim.build_optimizer(net, cfg, grad_clip=dict(max_norm=0.5))
    assert cfg == keep, "the config is not modified"
    assert isinstance(opt, optim.AdamW) and opt.max_norm == 0.5 and len(opt.param_groups) == len(names)
    got = {n: (g["lr"], g["weight_decay"]) for n, g in zip(names, opt.param_groups)}
    close = lambda a, b: all(math.isclose(x, y, rel_tol=1e-12, abs_tol=0) for x, y in zip(a, b))     # noqa: E731
    assert close(got["backbone.0.weight"], (1e-4, 0.1))            # decay_mult defaults to 1
    assert close(got["backbone.0.bias"], (1e-4, 0.1))              # "backbone" (8 letters) comes before "bias" (4)
    assert got["backbone.1.weight"] == (0.0, 0.0)                  # the longer key beats "backbone"
    assert close(got["encoder.weight"], (2e-3, 0.3))
    assert close(got["encoder.bias"], (2e-3, 0.3))                 # "encoder" (7) before "bias" (4)
    assert close(got["decoder.weight"], (1e-3, 0.1))               # no key matches: the defaults
    assert close(got["decoder.bias"], (1e-3, 0.1))                 # requires_grad False: the defaults, though "bias" matches
    assert all(g["betas"] == (0.9, 0.99) and g["eps"] == 1e-6 for g in opt.param_groups)
    # keys of equal length: alphabetical order decides
    tie = optim.build_optimizer(net, dict(type="Adam", lr=1.0, paramwise_cfg=dict(
        custom_keys={"weight": dict(lr_mult=3.0), "encode": dict(lr_mult=5.0)})))
    assert {n: g["lr"] for n, g in zip(names, tie.param_groups)}["encoder.weight"] == 5.0
    # without a weight decay in the config decay_mult has nothing to multiply
    nowd = optim.build_optimizer(net, dict(type="Adam", lr=1.0, paramwise_cfg=dict(custom_keys={"bias": dict(decay_mult=0.0)})))
    assert all(g["weight_decay"] == 0.0 for g in nowd.param_groups)
    # the torch backend: the torch.optim class of that name with the same groups
    ref = optim.build_optimizer(net, cfg, backend="torch")
    assert type(ref) is torch.optim.AdamW and len(ref.param_groups) == len(opt.param_groups)
    for a, b in zip(ref.param_groups, opt.param_groups):
        assert a["params"] == b["params"] and all(a[k] == b[k] for k in ("lr", "weight_decay", "betas", "eps"))
    assert type(optim.build_optimizer(net, dict(type="Adam", lr=1e-4), backend="torch")) is torch.optim.Adam


def test_build_optimizer_refuses_what_it_does_not_implement():
    net = _Net()
    for cfg, word in ((dict(type="SGD", lr=0.1), "SGD"), (dict(type="Adadelta", lr=1.0), "Adadelta"), (dict(lr=1.0), "None"),
                      (dict(type="Adam", lr=1.0, paramwise_cfg=dict(bias_lr_mult=2.0)), "bias_lr_mult"),
                      (dict(type="Adam", lr=1.0, paramwise_cfg=dict(custom_keys={}, norm_decay_mult=0.0)), "norm_decay_mult"),
                      (dict(type="Adam", lr=1.0, paramwise_cfg=dict(custom_keys={"a": dict(lr_mul=1.0)})), "lr_mul"),
                      (dict(type="Adam", lr=1.0, momentum=0.9), "momentum")):
        with pytest.raises(NotImplementedError, match=word):
            optim.build_optimizer(net, cfg)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        optim.build_optimizer(net, dict(type="Adam", lr=1.0, amsgrad=True))
    with pytest.raises(ValueError, match="backend"):
        optim.build_optimizer(net, dict(type="Adam", lr=1.0), backend="cuda")
    with pytest.raises(ValueError, match="clip_grad_norm_"):
        optim.build_optimizer(net, dict(type="Adam", lr=1.0), backend="torch", grad_clip=dict(max_norm=1.0))


def test_state_dict_round_trips_through_torch_adam():
    """State built on CPU tensors without stepping: torch's keys and types, so torch.optim.Adam takes it, steps with it,
    and hands it back."""
    params = [torch.nn.Parameter(torch.arange(4.0)), torch.nn.Parameter(torch.ones(2, 3))]
    hip = optim.Adam([dict(params=params[:1], lr=1e-2), dict(params=params[1:], weight_decay=0.1)], lr=1e-3)
    for i, p in enumerate(params):
        hip.state[p] = dict(step=torch.tensor(3.0), exp_avg=torch.full_like(p, 0.5 + i), exp_avg_sq=torch.full_like(p, 2.0 + i))
    sd = hip.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["state"][0]["step"].dtype == torch.float32
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.Adam([dict(params=clones[:1]), dict(params=clones[1:])], lr=7.0, foreach=False)
    ref.load_state_dict(sd)
    assert [g["lr"] for g in ref.param_groups] == [1e-2, 1e-3] and ref.param_groups[1]["weight_decay"] == 0.1
    for i, p in enumerate(clones):
        assert torch.equal(ref.state[p]["exp_avg"], torch.full_like(p, 0.5 + i)) and float(ref.state[p]["step"]) == 3
        p.grad = torch.ones_like(p)
    ref.step()                                                       # torch computes with the loaded state
    assert float(ref.state[clones[0]]["step"]) == 4
    back = optim.Adam([dict(params=params[:1]), dict(params=params[1:])], lr=9.0)
    back.load_state_dict(ref.state_dict())
    for p, q in zip(params, clones):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(back.state[p][k], ref.state[q][k]) and back.state[p][k].dtype == torch.float32, k
    assert [g["lr"] for g in back.param_groups] == [1e-2, 1e-3] and back.param_groups[1]["weight_decay"] == 0.1
    # an LR scheduler drives the groups as it drives torch's
    sched = torch.optim.lr_scheduler.LinearLR(back, start_factor=0.001, total_iters=10)
    assert math.isclose(back.param_groups[0]["lr"], 1e-5, rel_tol=1e-9) and sched.get_last_lr()[1] == pytest.approx(1e-6)


def test_parse_losses_follows_the_reference():
    parse = EncodeDecodeRecognizer._parse_losses
    a = torch.tensor([1.0, 3.0], requires_grad=True)
    loss, log_vars = parse(None, dict(loss_ce=a, acc=torch.tensor([0.25, 0.75]), loss_aux=[torch.tensor([2.0, 4.0]), torch.tensor(5.0)]))
    assert loss.requires_grad and float(loss.detach()) == 2.0 + 3.0 + 5.0                 # 'acc' is logged, not summed
    assert list(log_vars) == ["loss_ce", "acc", "loss_aux", "loss"]
    assert log_vars == dict(loss_ce=2.0, acc=0.5, loss_aux=8.0, loss=10.0)
    assert all(type(v) is float for v in log_vars.values())
    for bad in (1.0, (torch.tensor(1.0),), None):
        with pytest.raises(TypeError, match="loss_x is not a tensor or list of tensors"):
            parse(None, dict(loss_x=bad))
    for name in ("train_step", "val_step"):
        assert callable(getattr(EncodeDecodeRecognizer, name))


@pytest.mark.parametrize("case", list(TG.CASES))
def test_torchs_own_error_on_the_gpu_tests_inputs_is_below_its_cap(case):
    """The bar of tests/test_gpu_optim.py is twice torch.optim's own fp32 error: here that error is held under the caps, on
    the machine that has no GPU as well."""
    base = TG.run_case(TG.torch_class(case), "cpu", case)[0]
    print(case, base)
    for b, cap in zip(base, TG.CAPS[case]):
        assert math.isfinite(b) and 0 < b < cap
