"""GPU tests of the optimiser stage (tps_pp_amd/optim.py, include/tpspp_train_opt.h): the multi-tensor Adam / AdamW update
against an fp64 reference in rounding units with torch.optim's own fp32 error as the bar, exact zeros, guard bands, bitwise
reproducibility, the gradient norm and clipping without a host synchronisation, torch's optimiser semantics, the
prepared-weight cache after a step, and a whole train_step -> backward -> step iteration of the small recogniser.

The helpers at the top run on any device: tests/test_optim_host.py uses them on the CPU to hold torch's own error
figures under the caps stated in CAPS."""
import math

import pytest
import torch

import guarded_alloc as GA
from tps_pp_amd import optim

EPS = 2.0 ** -23
CHUNK = optim.CHUNK
SIZES = [1, 2, 3, 18, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
UNALIGNED = 4                      # index into SIZES of the tensor that starts one element into its storage
LR, BETAS, ADAM_EPS = 1e-2, (0.9, 0.999), 1e-8
CASES = {                          # name: (class name, weight decay, per-tensor lr multipliers or None)
    "adam": ("Adam", 0.0, None),
    "adam_wd": ("Adam", 1e-4, None),
    "adamw": ("AdamW", 1e-2, None),
    "adam_lr_mult": ("Adam", 0.0, (0.0, 0.1, 1.0)),
}
# Caps on torch.optim's own maxima (m, v, p units) on the CPU, so that a broken baseline cannot widen the bar.  Plain Adam:
# 8 units.  The two weight-decay cases: twice what torch.optim(foreach=False) measured on the CPU on these inputs, m / v / p:
# adam_wd 0.49 / 1.06 / 13.24 (where g + wd p cancels, the rounding of g' reaches p through m / sqrt(v)), adamw 0.48 / 1.02 /
# 3.07.
CAPS = {"adam": (8.0, 8.0, 8.0), "adam_lr_mult": (8.0, 8.0, 8.0), "adam_wd": (0.99, 2.12, 26.5), "adamw": (0.97, 2.04, 6.15)}
# clip_grad_norm_(max_norm=1) + plain Adam: torch measured 0.49 / 1.03 / 23.03 (the clipped gradients are so small that
# sqrt(v) falls below Adam's eps, and the fp32 rounding of the scaled gradient shows in p); m and v keep the cap of 8, p gets
# twice torch's figure
CLIP_CAPS = (8.0, 8.0, 46.1)


def log_uniform(shape, lo, hi, gen):
    mag = torch.exp(torch.rand(shape, generator=gen, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))
    sign = torch.where(torch.rand(shape, generator=gen) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


def make_inputs(seed=0, steps=4, sizes=SIZES):
    """Parameters 1e-3 .. 1e1 and `steps` sets of gradients 1e-6 .. 1e2 in magnitude, both signs, every seventh gradient
    exactly 0 (CPU fp32 tensors)."""
    gen = torch.Generator().manual_seed(seed)
    params = [log_uniform((n,), 1e-3, 1e1, gen) for n in sizes]
    grads = []
    for _ in range(steps):
        gs = [log_uniform((n,), 1e-6, 1e2, gen) for n in sizes]
        for g in gs:
            g[::7] = 0.0
        grads.append(gs)
    return params, grads


def reference_step(p0, g, m0, v0, t, lr, wd, kind, coef=1.0):
    """One Adam / AdamW step in fp64 from the fp32 state (p0, m0, v0) and gradient g."""
    b1, b2 = BETAS
    p0, g, m0, v0 = p0.double().cpu(), g.double().cpu() * coef, m0.double().cpu(), v0.double().cpu()
    p = p0
    if kind == "Adam" and wd:
        g = g + wd * p0
    if kind == "AdamW":
        p = p0 * (1.0 - lr * wd)
    m = m0 + (1.0 - b1) * (g - m0)
    v = b2 * v0 + (1.0 - b2) * g * g
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** t) + ADAM_EPS
    return p - lr / (1.0 - b1 ** t) * (m / denom), m, v


def units(before, after, g, ref, wd):
    """Maximum error of (m, v, p) in rounding units that do not cancel:
       |m - m64| / (eps (|m0| + |g| + wd |p0|)),  |v - v64| / (eps (v0 + (|g| + wd |p0|)^2)),
       |p - p64| / (eps (|p0| + |dp64|)).  Where a scale is 0 the result must be exact."""
    p0, m0, v0 = (x.double().cpu() for x in before)
    p1, m1, v1 = (x.double().cpu() for x in after)
    p64, m64, v64 = ref
    ga = g.double().cpu().abs() + wd * p0.abs()
    out = []
    for got, want, scale in ((m1, m64, m0.abs() + ga), (v1, v64, v0 + ga * ga), (p1, p64, p0.abs() + (p64 - p0).abs())):
        err = (got - want).abs()
        assert torch.isfinite(err).all()
        assert (err[scale == 0] == 0).all()
        ok = scale > 0
        out.append(float((err[ok] / (EPS * scale[ok])).max()) if ok.any() else 0.0)
    return out


def groups_for(params, mults):
    if mults is None:
        return [dict(params=params)]
    return [dict(params=[p], lr=LR * mults[i % len(mults)]) for i, p in enumerate(params)]


def run_case(make_optimizer, device, case, steps=4, coef_of=None, pre_step=None):
    """`steps` steps of the optimiser `make_optimizer(groups, lr=, betas=, eps=, weight_decay=)` on `device`; before each
    step the fp64 reference restarts from the optimiser's own fp32 state.  Returns (maxima of (m, v, p) units over all
    steps and tensors, parameters, optimiser).  coef_of(grads) -> the fp64 clip coefficient of a step (None: 1);
    pre_step(params): what the baseline does between backward and step (clip_grad_norm_)."""
    kind, wd, mults = CASES[case]
    p_cpu, g_cpu = make_inputs()
    params = []
    for i, p in enumerate(p_cpu):
        if i == UNALIGNED:                                      # a view one element into its storage: 4-byte aligned only
            base = torch.zeros(p.numel() + 1, device=device)
            base[1:] = p.to(device)
            params.append(torch.nn.Parameter(base[1:]))
            assert params[-1].data_ptr() % 16 == 4
        else:
            params.append(torch.nn.Parameter(p.to(device)))
    opt = make_optimizer(groups_for(params, mults), lr=LR, betas=BETAS, eps=ADAM_EPS, weight_decay=wd)
    worst = [0.0, 0.0, 0.0]
    for t in range(1, steps + 1):
        for p, g in zip(params, g_cpu[t - 1]):
            p.grad = g.clone().to(device)
        coef = 1.0 if coef_of is None else coef_of([p.grad for p in params])
        before = []
        for p in params:
            st = opt.state.get(p, {})
            zero = torch.zeros_like(p)
            before.append((p.detach().clone(), st["exp_avg"].clone() if st else zero, st["exp_avg_sq"].clone() if st else zero))
        if pre_step is not None:
            pre_step(params)
        opt.step()
        for i, (p, b) in enumerate(zip(params, before)):
            lr = opt.param_groups[i if mults is not None else 0]["lr"]
            ref = reference_step(b[0], g_cpu[t - 1][i], b[1], b[2], t, lr, wd, kind, coef)
            st = opt.state[p]
            assert float(st["step"]) == t
            u = units(b, (p.detach(), st["exp_avg"], st["exp_avg_sq"]), g_cpu[t - 1][i] * coef, ref, wd)
            worst = [max(a, c) for a, c in zip(worst, u)]
            if lr == 0.0:                                       # lr_mult = 0: p bit-unchanged while m and v moved
                assert GA.same_bits(p.detach(), b[0])[0], f"tensor {i}: lr = 0 changed the parameter"
                if g_cpu[t - 1][i].count_nonzero():             # (the one-element tensor's only gradient is an exact 0)
                    assert not torch.equal(st["exp_avg"], b[1]) and not torch.equal(st["exp_avg_sq"], b[2])
    return worst, params, opt


def torch_class(case):
    kind = CASES[case][0]
    cls = torch.optim.Adam if kind == "Adam" else torch.optim.AdamW
    return lambda groups, **kw: cls(groups, foreach=False, **kw)


def hip_class(case, **extra):
    cls = optim.Adam if CASES[case][0] == "Adam" else optim.AdamW
    return lambda groups, **kw: cls(groups, **kw, **extra)


def check_bar(case, hip, base, caps=None):
    print(f"{case}: units m / v / p  hip {hip[0]:.3f} / {hip[1]:.3f} / {hip[2]:.3f}   "
          f"torch cpu {base[0]:.3f} / {base[1]:.3f} / {base[2]:.3f}")
    for name, b, cap in zip("mvp", base, caps or CAPS[case]):
        assert math.isfinite(b) and b < cap, f"{case}: torch's own {name} error {b} units is not below {cap}"
    for name, h, b in zip("mvp", hip, base):
        assert h <= 2.0 * b, f"{case}: {name} error {h:.3f} units > 2 x torch's {b:.3f}"


pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def baselines():
    """torch.optim(foreach=False) in fp32 on the CPU on the same inputs, in the same units: computed once, shared."""
    return {case: run_case(torch_class(case), "cpu", case)[0] for case in CASES}


# ---- 1. arithmetic -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
def test_update_is_within_twice_torchs_own_rounding_error(cuda, baselines, case):
    hip, _, _ = run_case(hip_class(case), cuda, case)
    check_bar(case, hip, baselines[case])


# ---- 2. exact zeros ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["Adam", "AdamW"])
def test_zero_gradient_and_zero_state_leave_the_parameter_bit_unchanged(cuda, kind):
    p_cpu, _ = make_inputs()
    p_cpu[2][1] = -0.0
    params = [torch.nn.Parameter(p.to(cuda)) for p in p_cpu]
    for p in params:
        p.grad = torch.zeros_like(p)
    opt = getattr(optim, kind)(params, lr=LR, weight_decay=0.0)
    opt.step()
    for p, want in zip(params, p_cpu):
        assert GA.same_bits(p.detach().cpu(), want)[0]
        for k in ("exp_avg", "exp_avg_sq"):
            assert (opt.state[p][k].view(torch.int32) == 0).all(), k       # +0.0, not -0.0


# ---- 3. memory safety ----------------------------------------------------------------------------------------------------
def test_guards_hold_and_gradients_are_only_read(cuda):
    p_cpu, g_cpu = make_inputs(steps=1)
    with GA.guarded(cuda) as g:
        params = []
        for i, (p, gr) in enumerate(zip(p_cpu, g_cpu[0])):
            if i == UNALIGNED:
                params.append(torch.nn.Parameter(g.input(torch.cat([p[:1], p]))[1:]))
            else:
                params.append(torch.nn.Parameter(g.input(p)))
            # the gradient of the tensor after it is the one that is 4-byte aligned only
            params[-1].grad = g.input(torch.cat([gr[:1], gr]))[1:] if i == UNALIGNED + 1 else g.input(gr)
        assert params[UNALIGNED].data_ptr() % 16 == 4 and params[UNALIGNED + 1].grad.data_ptr() % 16 == 4
        grads = [p.grad.clone() for p in params]
        served = g.allocations()
        plain = optim.Adam(params, lr=LR, weight_decay=1e-4)
        plain.step()
        state = [plain.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")]
        g.check(state + [plain._table, plain._map, plain._scalars], require_guarded=True)
        assert g.allocations() - served == 2 * len(params) + 3
        clipped = optim.AdamW(params, lr=LR, grad_clip=dict(max_norm=1.0))
        clipped.step()
        g.check([clipped.state[p][k] for p in params for k in ("exp_avg", "exp_avg_sq")] +
                [clipped._table, clipped._map, clipped._scalars, clipped._partials, clipped.grad_clip_state],
                require_guarded=True)
        assert not g.fallthrough, g.fallthrough
        ok, why = GA.same_bits([p.grad for p in params], grads)
        assert ok, "step() wrote a gradient: " + why
        assert all(torch.isfinite(p).all() for p in params)
        clipped.zero_grad(set_to_none=False)
        g.check()
        for p in params:
            assert (p.grad.view(torch.int32) == 0).all()
        assert clipped.table_builds == 1


# ---- 4. reproducibility --------------------------------------------------------------------------------------------------
def test_two_runs_and_a_tensor_alone_give_the_same_bits(cuda):
    def run(pick=None):
        p_cpu, g_cpu = make_inputs(steps=2)
        idx = range(len(p_cpu)) if pick is None else pick
        params = [torch.nn.Parameter(p_cpu[i].to(cuda)) for i in idx]
        opt = optim.Adam(params, lr=LR, weight_decay=1e-4, grad_clip=dict(max_norm=1e9))
        norms = []
        for t in range(2):
            for p, i in zip(params, idx):
                p.grad = g_cpu[t][i].to(cuda)
            opt.step()
            norms.append(opt.last_grad_norm.clone())
        return [[p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"]] for p in params], norms
    a, na = run()
    b, nb = run()
    assert GA.same_bits(a, b)[0] and GA.same_bits(na, nb)[0]
    for i in (0, 4, len(SIZES) - 1):
        alone, _ = run([i])
        ok, why = GA.same_bits(alone[0], a[i])
        assert ok, f"tensor {i} alone differs from the same tensor inside the set: {why}"


# ---- 5. clipping ---------------------------------------------------------------------------------------------------------
def norm64(grads):
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def test_norm_matches_fp64_and_a_loose_bound_changes_nothing(cuda):
    """Tolerance of the norm: a chunk's partial is a sum of non-negative fp32 terms of depth CHUNK / THREADS (one thread,
    fma) + 6 (butterfly) + THREADS / 64 - 1 (wavefronts) roundings of 2^-24 each at most, the fp64 sum of the partials
    adds nothing visible, the square root halves the relative error and the result is rounded once more to fp32."""
    depth = CHUNK // optim.THREADS + 6 + optim.THREADS // 64 - 1
    tol = (depth / 2 + 1) * 2.0 ** -24
    loose, _, opt = run_case(hip_class("adam", grad_clip=dict(max_norm=1e9)), cuda, "adam")
    assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dim() == 0
    _, g_cpu = make_inputs()
    want = norm64(g_cpu[3])
    got, coef, flag = opt.grad_clip_state.tolist()
    print(f"norm {got!r} against fp64 {want!r}: relative error {abs(got - want) / want:.3e}, tolerance {tol:.3e}")
    assert abs(got - want) <= tol * want and coef == 1.0 and flag == 0.0
    plain, params, _ = run_case(hip_class("adam"), cuda, "adam")
    _, clipped, _ = run_case(hip_class("adam", grad_clip=dict(max_norm=1e9)), cuda, "adam")
    assert GA.same_bits([p.detach() for p in params], [p.detach() for p in clipped])[0]
    assert loose == plain


def test_clipped_step_matches_clip_grad_norm_and_torch_adam(cuda):
    max_norm = 1.0

    def coef64(grads):
        return min(1.0, max_norm / (norm64([g.cpu() for g in grads]) + 1e-6))

    def clip(params):
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    base, _, _ = run_case(torch_class("adam"), "cpu", "adam", coef_of=coef64, pre_step=clip)
    hip, params, opt = run_case(hip_class("adam", grad_clip=dict(max_norm=max_norm)), cuda, "adam", coef_of=coef64)
    assert opt.grad_clip_state[1].item() < 1e-2                  # the gradients are far above the bound: really clipped
    _, g_cpu = make_inputs()
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(params, g_cpu[3])), "gradients are left unscaled"
    check_bar("adam", hip, base, CLIP_CAPS)


def test_step_with_clipping_does_not_synchronise(cuda):
    p_cpu, g_cpu = make_inputs(steps=2)
    params = [torch.nn.Parameter(p.to(cuda)) for p in p_cpu]
    opt = optim.Adam(params, lr=LR, grad_clip=dict(max_norm=1.0))
    for t in range(2):                                           # the first step builds the table, the second reuses it
        grads = [g.to(cuda) for g in g_cpu[t]]
        torch.cuda.synchronize()
        for p, g in zip(params, grads):
            if t == 0:
                p.grad = g
            else:
                p.grad.copy_(g)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            opt.step()
            opt.zero_grad(set_to_none=False)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert opt.table_builds == 1 and opt.last_grad_norm.is_cuda
    with pytest.raises(NotImplementedError, match="norm_type"):
        optim.Adam(params, grad_clip=dict(max_norm=1.0, norm_type=1))


# ---- 6. torch semantics --------------------------------------------------------------------------------------------------
def test_skipped_parameters_lr_changes_and_replaced_gradients(cuda):
    p_cpu, g_cpu = make_inputs(steps=3, sizes=[5, 300, 7])
    params = [torch.nn.Parameter(p.to(cuda)) for p in p_cpu]
    opt = optim.Adam([dict(params=params[:2]), dict(params=params[2:])], lr=LR)
    ref = torch.optim.Adam([torch.nn.Parameter(p.clone()) for p in p_cpu[:2]], lr=LR, foreach=False)
    for p, q, g in zip(params, ref.param_groups[0]["params"], g_cpu[0]):
        p.grad, q.grad = g.to(cuda), g.clone()
    params[2].grad = None
    frozen = params[2].detach().clone()
    opt.step()
    ref.step()
    assert params[2] not in opt.state and torch.equal(params[2].detach(), frozen)      # no gradient: no state, no step
    assert float(opt.state[params[0]]["step"]) == 1 and opt.table_builds == 1
    # a new lr takes effect without a rebuild (gradients updated in place, as backward() accumulates into zeroed ones)
    opt.param_groups[0]["lr"] = ref.param_groups[0]["lr"] = LR * 0.25
    for p, q, g in zip(params, ref.param_groups[0]["params"], g_cpu[1]):
        p.grad.copy_(g)
        q.grad.copy_(g)
    uploads = opt.scalar_uploads
    opt.step()
    ref.step()
    assert opt.table_builds == 1 and opt.scalar_uploads == uploads + 1
    for p, q in zip(params, ref.param_groups[0]["params"]):
        # the quarter step: with the old lr the parameters would be 0.75 * LR further along
        assert torch.allclose(p.detach().cpu(), q.detach(), rtol=1e-5, atol=1e-7)
    # replacing one .grad tensor: exactly one rebuild
    params[0].grad = g_cpu[2][0].to(cuda)
    opt.step()
    opt.step()
    assert opt.table_builds == 2
    # what the kernels cannot take raises before any launch and names the parameter
    named = optim.build_optimizer(torch.nn.Linear(3, 2).to(cuda).half(), dict(type="Adam", lr=LR))
    for p in named.param_groups[0]["params"]:
        p.grad = torch.zeros_like(p)
    with pytest.raises(Exception, match="weight must be a dense contiguous fp32"):
        named.step()


# ---- 7. the prepared-weight cache ----------------------------------------------------------------------------------------
def test_hip_forward_after_a_step_uses_the_updated_weights(cuda):
    """Fails without the version bump after the launch: the second forward would reuse the layouts prepared from the old
    weights and return the first forward's bits."""
    from tps_pp_amd import TPS_PP
    torch.manual_seed(3)
    m = TPS_PP().to(cuda).eval()
    x = torch.rand(1, 64, 16, 64, device=cuda)
    outs = [torch.rand(1, 32, 32, 128, device=cuda), torch.rand(1, 32, 32, 128, device=cuda)]
    with torch.no_grad():
        first = m(x, outs)["output"].clone()
    versions = [p._version for p in m.parameters()]
    for p in m.parameters():
        p.grad = torch.randn_like(p)
    optim.Adam(m.parameters(), lr=1e-2).step()
    assert all(p._version > v for p, v in zip(m.parameters(), versions))
    with torch.no_grad():
        second = m(x, outs)["output"].clone()
        fresh = TPS_PP().to(cuda).eval()
        fresh.load_state_dict(m.state_dict())
        want = fresh(x, outs)["output"]
    assert not torch.equal(first, second), "the forward after step() still computes with the old weights"
    ok, why = GA.same_bits(second, want)
    assert ok, "stale prepared weights after step(): " + why


# ---- 8. a whole iteration ------------------------------------------------------------------------------------------------
def test_train_step_backward_step_on_the_small_recogniser(cuda):
    from test_attn_train_host import small_recogniser
    torch.manual_seed(0)
    init = {k: v.clone() for k, v in small_recogniser().state_dict().items()}
    img = torch.randn((2, 3, 32, 128), device=cuda)

    def data():
        return dict(img=img, img_metas=[dict(resize_shape=(32, 128, 3), text="ab"), dict(resize_shape=(32, 100, 3), text="tps")])

    def fresh():
        m = small_recogniser()
        m.load_state_dict(init)
        return m.to(cuda).train()

    def run(make):
        m = fresh()
        opt = make(m)
        losses, grads = [], []
        for it in range(3):
            torch.manual_seed(100 + it)
            out = m.train_step(data(), opt)
            assert set(out) == {"loss", "log_vars", "num_samples"} and out["num_samples"] == 2
            assert isinstance(out["log_vars"]["loss"], float) and out["loss"].requires_grad
            opt.zero_grad()
            out["loss"].backward()
            grads.append([None if p.grad is None else p.grad.detach().clone() for p in m.parameters()])
            opt.step()
            losses.append(out["log_vars"]["loss"])
        with torch.no_grad():
            torch.manual_seed(7)
            val = m.val_step(data(), None)
        assert set(val) == {"loss", "log_vars", "num_samples"} and isinstance(val["log_vars"]["loss"], float)
        return losses, [p.detach().clone() for p in m.parameters()], grads

    def dist(a, b):
        return max(float((x.double() - y.double()).abs().max()) for x, y in zip(a, b))

    lr = 1e-4
    t_loss, t_par, t_grads = run(lambda m: torch.optim.Adam(m.parameters(), lr=lr, foreach=False))
    t2_loss, t2_par, _ = run(lambda m: torch.optim.Adam(m.parameters(), lr=lr, foreach=False))
    h_loss, h_par, _ = run(lambda m: optim.build_optimizer(m, dict(type="Adam", lr=lr)))
    assert h_loss[0] == t_loss[0], "iteration 1 runs on identical weights: identical loss"
    # fp32 against fp64 torch Adam over the same three steps, fed the first torch run's gradients
    p0 = [p.detach() for p in fresh().parameters()]
    p32 = [torch.nn.Parameter(p.clone()) for p in p0]
    p64 = [torch.nn.Parameter(p.double()) for p in p0]
    o32 = torch.optim.Adam(p32, lr=lr, foreach=False)
    o64 = torch.optim.Adam(p64, lr=lr, foreach=False)
    for gs in t_grads:
        for a, b, g in zip(p32, p64, gs):
            a.grad, b.grad = (None, None) if g is None else (g.clone(), g.double())
        o32.step()
        o64.step()
    run_to_run = dist(t_par, t2_par)
    precision = dist([p.detach() for p in p32], [p.detach() for p in p64])
    got = dist(h_par, t_par)
    print(f"HIP Adam against torch Adam after 3 iterations: {got:.3e}; torch run to run {run_to_run:.3e}; "
          f"torch fp32 against fp64 {precision:.3e}; losses hip {h_loss} torch {t_loss}")
    assert math.isfinite(got) and got <= 4.0 * max(run_to_run, precision)
