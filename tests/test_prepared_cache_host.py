"""CPU tests of the one cache of prepared kernel weights (tps_pp_amd/_prepared.py): when a slot is rebuilt, that slots do
not disturb each other, and that a populated cache is invisible to state_dict() / parameters().  The builders are plain
Python callables that count their calls: no library, no GPU."""
import json
import os

import torch
import torch.nn as nn

import cases
from tps_pp_amd import TPS_PP
from tps_pp_amd._prepared import invalidate_prepared, prepared


class Counter:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return self.calls


def small():
    torch.manual_seed(0)
    return nn.Sequential(nn.Conv2d(3, 4, 3, bias=True), nn.BatchNorm2d(4))


def slots_of(module):
    return [m for m in module.modules() if m.__dict__.get("_tpspp_prepared")]


def test_second_call_does_not_rebuild_and_returns_the_same_object():
    m, build = small(), Counter()
    obj = object()
    assert prepared(m, "w", [m], lambda: obj) is obj
    assert prepared(m, "w", [m], build) is obj and build.calls == 0
    assert prepared(m, "w", [m], build) is obj and build.calls == 0


def test_rebuilds_after_an_in_place_update_and_an_optimiser_step():
    m, build = small(), Counter()
    prepared(m, "w", [m], build)
    with torch.no_grad():
        m[0].weight.mul_(2.0)
    assert prepared(m, "w", [m], build) == 2
    assert prepared(m, "w", [m], build) == 2
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    m(torch.randn(2, 3, 8, 8)).sum().backward()
    prepared(m, "w", [m], build)                # (the training forward moved the BatchNorm buffers)
    n = build.calls
    opt.step()
    assert prepared(m, "w", [m], build) == n + 1
    assert prepared(m, "w", [m], build) == n + 1


def test_rebuilds_after_load_state_dict():
    m, build = small(), Counter()
    prepared(m, "w", [m], build)
    m.load_state_dict({k: v.clone() for k, v in m.state_dict().items()})
    assert prepared(m, "w", [m], build) == 2


def test_rebuilds_when_a_batchnorm_buffer_changes():
    m, build = small(), Counter()
    prepared(m, "w", [m], build)
    m[1].running_mean.copy_(torch.ones(4))
    assert prepared(m, "w", [m], build) == 2
    # a site that names the tensors it depends on sees exactly those
    prepared(m, "conv", [m[0].weight, m[0].bias, None], build)
    n = build.calls
    m[1].running_var.copy_(torch.full((4,), 2.0))
    assert prepared(m, "conv", [m[0].weight, m[0].bias, None], build) == n


def test_rebuilds_after_to_and_parameter_replacement():
    m, build = small(), Counter()
    prepared(m, "w", [m], build)
    m.to(torch.float64)                          # new storage behind every parameter and buffer
    assert prepared(m, "w", [m], build) == 2
    m[0].weight = nn.Parameter(m[0].weight.detach().clone())
    assert prepared(m, "w", [m], build) == 3
    assert prepared(m, "w", [m], build) == 3


def test_rebuilds_when_the_configuration_changes():
    m, build = small(), Counter()
    assert prepared(m, "w", [m], build, config=(("x3", False),)) == 1
    assert prepared(m, "w", [m], build, config=(("x3", False),)) == 1
    assert prepared(m, "w", [m], build, config=(("x3", True),)) == 2
    assert prepared(m, "w", [m], build, config=(("x3", True),)) == 2


def test_two_slots_on_one_module_do_not_disturb_each_other():
    m, a, b = small(), Counter(), Counter()
    prepared(m, "a", [m[0]], a)
    prepared(m, ("train", "b"), [m[1]], b)
    m[1].running_mean.copy_(torch.ones(4))
    prepared(m, "a", [m[0]], a)
    prepared(m, ("train", "b"), [m[1]], b)
    assert (a.calls, b.calls) == (1, 2)
    prepared(m, "a", [m[0]], a, config="other")
    prepared(m, ("train", "b"), [m[1]], b)
    assert (a.calls, b.calls) == (2, 2)


def test_invalidating_a_parent_drops_its_childrens_slots():
    m, top, child = small(), Counter(), Counter()
    prepared(m, "w", [m], top)
    prepared(m[0], "w", [m[0]], child)
    assert len(slots_of(m)) == 2
    assert invalidate_prepared(m) is m and slots_of(m) == []
    prepared(m, "w", [m], top)
    prepared(m[0], "w", [m[0]], child)
    assert (top.calls, child.calls) == (2, 2)
    invalidate_prepared(m[1])                    # a sibling's invalidation leaves them alone
    prepared(m[0], "w", [m[0]], child)
    assert child.calls == 2


def test_a_populated_cache_is_invisible_to_state_dict_and_parameters():
    m = TPS_PP()
    keys = json.load(open(os.path.join(cases.HERE, "state_dict_keys.json")))["TPS_PP"]
    before_keys, before_params = list(m.state_dict()), [id(p) for p in m.parameters()]
    before_buffers, before_modules = [id(b) for b in m.buffers()], [n for n, _ in m.named_modules()]
    for owner in (m, m.atten_tps, m.down1):
        prepared(owner, "w", [owner], lambda: torch.zeros(3))
        prepared(owner, ("train", "x"), [m.down1.conv.weight], lambda: nn.Linear(2, 2))
    assert list(m.state_dict()) == before_keys == list(keys)
    assert [id(p) for p in m.parameters()] == before_params
    assert [id(b) for b in m.buffers()] == before_buffers
    assert [n for n, _ in m.named_modules()] == before_modules


def test_rewiring_leaves_no_slot_behind():
    m = TPS_PP()
    for owner in (m, m.down0, m.MSFA, m.atten_tps):
        prepared(owner, "w", [owner], Counter())
    assert len(slots_of(m)) == 4
    m.set_variant("ResNet45")
    assert m.type == "ResNet45" and slots_of(m) == []
