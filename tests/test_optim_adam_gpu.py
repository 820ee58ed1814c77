"""dgx.optim.Adam / AdamW (one-launch multi-tensor update, csrc/optim.hip), the
GradScaler protocol of dgx.optim.SGD / Adam / AdamW and dgx.optim.GradScaler,
against torch's own optimizers and scaler on the same parameters and gradients.

Every case uses one list of 60 tensors (two launches of <= 48): sizes 1, 3, 4,
1023, 1024, 1025, 4099 (around the 4-element vector and the 1024-element
piece), (64, 6), a zero-element tensor, a view that starts 4 bytes into its
buffer (not 16-byte aligned: the scalar path), a parameter whose gradient
appears from step 2 only, and odd sizes below 700.

The parity bar is measured, not chosen: the same quantities are computed
between torch's own single-tensor (foreach=False, fused=False) and fused forms,
and the engine may differ from the single-tensor form by twice that spread
(per quantity: the largest over tensors and steps), with a floor of 2^-20 (at
most eight fp32 roundings of 2^-24 per element and step, three steps of moment
error). Figures are max |a - b| / max |reference| per tensor.

Measured on an MI355X (torch 2.10, ROCm 7.0). torch single-tensor vs fused:
update 2.38e-5 for Adam (one ulp of a parameter of magnitude 2-4, seen through
an update of 1e-2) and 1.24e-4 for AdamW / decoupled decay, exp_avg 2.07e-7
(4.2e-7 with betas (0.8, 0.9)), exp_avg_sq and max_exp_avg_sq 1.5e-7 to 2.2e-7;
SGD: update 8.9e-7, momentum buffer 3.3e-7. Engine vs torch single-tensor:
update 2.38e-5 (Adam) and 2.39e-5 (AdamW), exp_avg 0, exp_avg_sq and
max_exp_avg_sq 1.4e-7 to 1.5e-7. Each case prints its figures (pytest -s)."""
import copy
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20
N_TENSORS = 60
I_1025, I_EMPTY, I_UNALIGNED, I_LATE = 5, 8, 9, 10
STEPS = 3

ADAM_SETTINGS = {
    "plain": ("Adam", dict(lr=1e-2)),
    "wd": ("Adam", dict(lr=1e-2, weight_decay=1e-4)),
    "amsgrad": ("Adam", dict(lr=1e-2, amsgrad=True)),
    "maximize": ("Adam", dict(lr=1e-2, maximize=True, betas=(0.8, 0.9))),
    "adamw": ("AdamW", dict(lr=1e-2, weight_decay=1e-2)),
    "decoupled": ("Adam", dict(lr=1e-2, weight_decay=1e-2, decoupled_weight_decay=True)),
}
SGD_KW = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)


# ---- the tensor list --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _host_values():
    """(initial values, per-step gradients) on the host, computed once."""
    g = torch.Generator(device="cpu").manual_seed(3)
    shapes = [(1,), (3,), (4,), (1023,), (1024,), (1025,), (4099,), (64, 6), (0,), (131,), (37,)]
    shapes += [(2 * int(torch.randint(1, 350, (1,), generator=g)) - 1,) for _ in range(N_TENSORS - len(shapes))]
    assert len(shapes) == N_TENSORS and shapes[I_1025] == (1025,) and shapes[I_EMPTY] == (0,)
    vals = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(5)]
    return vals, grads


def _place(t, dev, unaligned):
    """``t`` on the device; ``unaligned``: as a view 4 bytes into a larger buffer."""
    if not unaligned:
        return t.to(dev)
    buf = torch.empty(t.numel() + 1, device=dev)
    view = buf[1:]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _params(dev):
    vals, _ = _host_values()
    return [_place(v, dev, i == I_UNALIGNED).requires_grad_(True) for i, v in enumerate(vals)]


def _set_grads(params, step, dev, scale=1.0, late=True, static=False):
    """Gradients of ``step``; the late parameter has none on step 0 (``late``).
    ``static``: copy into the existing gradient buffers (graph replays)."""
    _, grads = _host_values()
    for i, (p, g) in enumerate(zip(params, grads[step])):
        if i == I_LATE and late and step == 0:
            continue
        if static:
            if p.grad is not None:
                p.grad.copy_(g.to(dev) * scale)
        else:
            p.grad = _place(g * scale, dev, i == I_UNALIGNED)


STATE_KEYS = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer", "step")


def _snapshot(opt, params):
    out = {"p": [p.detach().clone() for p in params]}
    for k in STATE_KEYS:
        out[k] = [opt.state[p][k].detach().clone().to(p.device) if k in opt.state.get(p, {}) else None for p in params]
    return out


def _run(make_opt, dev, steps=STEPS, stepper=None, scale=1.0, late=True):
    """``steps`` optimizer steps on a fresh copy of the list; per step the update
    p_after - p_before and a snapshot of parameters and state."""
    params = _params(dev)
    opt = make_opt(params)
    rec = []
    for s in range(steps):
        _set_grads(params, s, dev, scale, late)
        before = [p.detach().clone() for p in params]
        (stepper or (lambda o: o.step()))(opt)
        snap = _snapshot(opt, params)
        snap["upd"] = [a - b for a, b in zip(snap["p"], before)]
        rec.append(snap)
    return rec, opt, params


def _distance(rec, ref, keys=("upd", "exp_avg", "exp_avg_sq", "max_exp_avg_sq", "momentum_buffer")):
    """{quantity: largest over steps and tensors of max|a - b| / max|ref|}; ``step`` must be equal."""
    out = {}
    for k in keys:
        errs = []
        for a_step, b_step in zip(rec, ref):
            for a, b in zip(a_step[k], b_step[k]):
                assert (a is None) == (b is None), k
                if a is not None and a.numel():
                    errs.append((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
        if errs:
            out[k] = float(torch.stack(errs).max())
    for a_step, b_step in zip(rec, ref):
        for a, b in zip(a_step["step"], b_step["step"]):
            assert (a is None) == (b is None)
            if a is not None:
                assert float(a) == float(b), ("step", float(a), float(b))
    return out


_torch_cache = {}


def _torch_adam(dev, name):
    """torch's single-tensor and fused runs of a setting, and the bar they set."""
    if name not in _torch_cache:
        cls, kw = ADAM_SETTINGS[name]
        cls = getattr(torch.optim, cls)
        single = _run(lambda ps: cls(ps, foreach=False, fused=False, **kw), dev)[0]
        fused = _run(lambda ps: cls(ps, fused=True, **kw), dev)[0]
        spread = _distance(fused, single)
        _torch_cache[name] = (single, fused, spread)
    return _torch_cache[name]


def _torch_sgd(dev):
    """As _torch_adam. Every SGD case gives all gradients from step 1: torch's
    fused SGD takes either no momentum buffer or all of them (_fused_sgd), so it
    cannot run a list in which one parameter's first gradient comes later."""
    if "sgd" not in _torch_cache:
        single = _run(lambda ps: torch.optim.SGD(ps, foreach=False, fused=False, **SGD_KW), dev, late=False)[0]
        fused = _run(lambda ps: torch.optim.SGD(ps, fused=True, **SGD_KW), dev, late=False)[0]
        _torch_cache["sgd"] = (single, fused, _distance(fused, single))
    return _torch_cache["sgd"]


def _assert_within(dist, spread, what):
    print(f"{what}: engine {dist}  torch single-vs-fused {spread}")
    for k, d in dist.items():
        bar = max(2.0 * spread.get(k, 0.0), FLOOR)
        assert d <= bar, (what, k, d, bar)


def _bit_equal(rec_a, rec_b):
    for k in ("p",) + STATE_KEYS:
        for a, b in zip(rec_a[k], rec_b[k]):
            assert (a is None) == (b is None), k
            if a is not None:
                assert torch.equal(a, b), k


def _dgx(name):
    import dgx.optim
    return getattr(dgx.optim, name)


# ---- 1. parity --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(ADAM_SETTINGS))
def test_adam_matches_torch(cuda, name):
    """Engine vs torch's single-tensor form, three steps, held to twice torch's
    own single-vs-fused spread (floor 2^-20). Measured on an MI355X: see
    DESIGN §8 (torch's spread, engine's distance)."""
    cls, kw = ADAM_SETTINGS[name]
    single, _, spread = _torch_adam(cuda, name)
    rec, opt, params = _run(lambda ps: _dgx(cls)(ps, **kw), cuda)
    _assert_within(_distance(rec, single), spread, name)
    st = opt.state[params[I_LATE]]["step"]
    assert st.is_cuda and st.dtype == torch.float32 and st.dim() == 0 and float(st) == STEPS - 1
    assert float(opt.state[params[I_EMPTY]]["step"]) == STEPS


# ---- 2. tensor lr -----------------------------------------------------------------------------------------------

def test_adam_tensor_lr(cuda):
    Adam = _dgx("Adam")
    lr = torch.tensor(1e-2, device=cuda)
    pf, pt, pk = _params(cuda), _params(cuda), _params(cuda)
    of, ot, ok = Adam(pf, lr=1e-2, weight_decay=1e-4), Adam(pt, lr=lr, weight_decay=1e-4), Adam(pk, lr=1e-2,
                                                                                                weight_decay=1e-4)
    for s in range(3):
        if s == 2:   # a scheduler's change: in place on the tensor, in the group for the float
            lr.fill_(3e-2)
            of.param_groups[0]["lr"] = 3e-2
        for ps, o in ((pf, of), (pt, ot), (pk, ok)):
            _set_grads(ps, s, cuda)
            o.step()
        _bit_equal(_snapshot(of, pf), _snapshot(ot, pt))
    assert not torch.equal(pt[I_1025], pk[I_1025])   # kept at 1e-2


# ---- 3. graph capture -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tensor_lr", [False, True])
def test_adam_graph_capture(cuda, tensor_lr):
    """One eager step, one captured step replayed three times with new gradients
    in the static buffers == four eager steps, bit for bit. The late parameter
    keeps no gradient here: its state would be created (zero-filled) inside the
    capture, and capture needs existing state."""
    Adam = _dgx("Adam")
    lrs = [1e-2, 1e-2, 2e-2, 5e-3]

    def lr_of():
        return torch.tensor(lrs[0], device=cuda) if tensor_lr else lrs[0]
    pe, pg = _params(cuda), _params(cuda)
    lr_e, lr_g = lr_of(), lr_of()
    oe, og = Adam(pe, lr=lr_e, amsgrad=True, weight_decay=1e-4), Adam(pg, lr=lr_g, amsgrad=True, weight_decay=1e-4)
    for s in range(4):
        _set_grads(pe, s, cuda)
        pe[I_LATE].grad = None
        if tensor_lr:
            lr_e.fill_(lrs[s])
        oe.step()
    _set_grads(pg, 0, cuda)
    og.step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    _set_grads(pg, 1, cuda, static=True)
    with torch.cuda.graph(graph):
        og.step()
    for s in range(1, 4):
        _set_grads(pg, s, cuda, static=True)
        if tensor_lr:
            lr_g.fill_(lrs[s])
        graph.replay()
    torch.cuda.synchronize()
    _bit_equal(_snapshot(og, pg), _snapshot(oe, pe))
    assert float(og.state[pg[0]]["step"]) == 4 and pg[I_LATE] not in og.state


# ---- 4. the scaler protocol -------------------------------------------------------------------------------------

SCALE = 2.0 ** 10


def _scaler(dev, cls=torch.amp.GradScaler):
    sc = cls("cuda", init_scale=SCALE)
    sc.scale(torch.zeros((), device=dev))   # the scale tensor is created by the first scale()
    return sc


def _scaled_stepper(sc):
    def stepper(opt):
        sc.step(opt)
        sc.update()
    return stepper


def test_scaler_step_adamw_vs_torch_fused(cuda):
    cls, kw = ADAM_SETTINGS["adamw"]
    _, _, spread = _torch_adam(cuda, "adamw")
    ref = _run(lambda ps: torch.optim.AdamW(ps, fused=True, **kw), cuda, stepper=_scaled_stepper(_scaler(cuda)),
               scale=SCALE)[0]
    sc = _scaler(cuda)
    rec = _run(lambda ps: _dgx("AdamW")(ps, **kw), cuda, stepper=_scaled_stepper(sc), scale=SCALE)[0]
    _assert_within(_distance(rec, ref), spread, "AdamW under GradScaler")
    assert sc.get_scale() == SCALE


def test_scaler_step_sgd_vs_torch_fused(cuda):
    _, _, spread = _torch_sgd(cuda)
    ref = _run(lambda ps: torch.optim.SGD(ps, fused=True, **SGD_KW), cuda, stepper=_scaled_stepper(_scaler(cuda)),
               scale=SCALE, late=False)[0]
    rec = _run(lambda ps: _dgx("SGD")(ps, **SGD_KW), cuda, stepper=_scaled_stepper(_scaler(cuda)), scale=SCALE,
               late=False)[0]
    _assert_within(_distance(rec, ref), spread, "SGD under GradScaler")


def test_scaler_step_sgd_bit_exact(cuda):
    """The scale is a power of two, so dividing the scaled gradient is exact:
    the scaler path equals the plain path on the unscaled gradients."""
    plain = _run(lambda ps: _dgx("SGD")(ps, **SGD_KW), cuda)[0]
    scaled = _run(lambda ps: _dgx("SGD")(ps, **SGD_KW), cuda, stepper=_scaled_stepper(_scaler(cuda)), scale=SCALE)[0]
    for a, b in zip(scaled, plain):
        _bit_equal(a, b)


@pytest.mark.parametrize("which", ["AdamW", "SGD"])
def test_scaler_skipped_step(cuda, which):
    """An inf in one gradient (data, not a fault): step/update leave every
    parameter, moment and step count bitwise unchanged and halve the scale; the
    next clean step equals torch's fused optimizer driven the same way. AdamW
    skips its very first step (state exists, all zero); SGD its second (torch's
    fused SGD leaves a first-step buffer uninitialised when that step is skipped)."""
    if which == "AdamW":
        kw, bad_step = ADAM_SETTINGS["adamw"][1], 0
        spread = _torch_adam(cuda, "adamw")[2]
        makers = (lambda ps: _dgx("AdamW")(ps, **kw)), (lambda ps: torch.optim.AdamW(ps, fused=True, **kw))
    else:
        kw, bad_step = SGD_KW, 1
        spread = _torch_sgd(cuda)[2]
        makers = (lambda ps: _dgx("SGD")(ps, **kw)), (lambda ps: torch.optim.SGD(ps, fused=True, **kw))
    recs = []
    for make in makers:
        params = _params(cuda)
        opt, sc = make(params), _scaler(cuda)
        rec = []
        for s in range(3):
            _set_grads(params, s, cuda, SCALE, late=False)
            if s == bad_step:
                params[I_1025].grad[7] = float("inf")
            before = _snapshot(opt, params)
            scale_before = sc.get_scale()
            sc.step(opt)
            sc.update()
            snap = _snapshot(opt, params)
            if s == bad_step:
                assert sc.get_scale() == scale_before / 2
                if make is makers[0]:
                    for k in ("p",) + STATE_KEYS:
                        for a, b in zip(snap[k], before[k]):
                            if b is not None:   # state created by the skipped step: zeros, step 0
                                assert torch.equal(a, b), k
                            elif a is not None:
                                assert not a.any(), k
            snap["upd"] = [a - b for a, b in zip(snap["p"], before["p"])]
            rec.append(snap)
        recs.append(rec)
    _assert_within(_distance(recs[0], recs[1]), spread, which + " around a skipped step")


def test_sgd_first_step_skipped(cuda):
    """A skipped first step creates the momentum buffers (as torch's fused SGD
    does) but writes nothing; they are zero, so the next step's buffer is g."""
    params = _params(cuda)
    opt, sc = _dgx("SGD")(params, **SGD_KW), _scaler(cuda)
    before = [p.detach().clone() for p in params]
    _set_grads(params, 0, cuda, SCALE, late=False)
    params[0].grad[0] = float("nan")
    sc.step(opt)
    sc.update()
    for p, b in zip(params, before):
        assert torch.equal(p.detach(), b) and not opt.state[p]["momentum_buffer"].any()
    _set_grads(params, 1, cuda, SCALE / 2, late=False)
    sc.step(opt)
    sc.update()
    p = params[I_1025]
    want = p.grad / (SCALE / 2) + SGD_KW["weight_decay"] * before[I_1025]
    assert torch.allclose(opt.state[p]["momentum_buffer"], want, rtol=1e-6, atol=0)


# ---- 5. dgx.optim.GradScaler -------------------------------------------------------------------------------------

def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


@pytest.mark.parametrize("inv", [1.0 / SCALE, 1.0])
@pytest.mark.parametrize("case", ["nan_last_unaligned", "inf_first_1025", "clean", "fp16_member", "fp16_inf"])
def test_grad_scaler_unscale_contract(cuda, case, inv):
    import types
    GradScaler = _dgx("GradScaler")
    outs = []
    for cls in (GradScaler, torch.amp.GradScaler):
        params = _params(cuda)
        _set_grads(params, 0, cuda, SCALE)
        assert params[I_UNALIGNED].grad.data_ptr() % 16 == 4
        if case == "nan_last_unaligned":
            params[I_UNALIGNED].grad[-1] = float("nan")
        elif case == "inf_first_1025":
            params[I_1025].grad[0] = float("-inf")
        elif case.startswith("fp16"):
            h = torch.arange(33, device=cuda, dtype=torch.float16).requires_grad_(True)
            h.grad = torch.arange(33, device=cuda, dtype=torch.float16) * 8
            if case == "fp16_inf":
                h.grad[5] = float("inf")
            params.insert(20, h)
        opt = types.SimpleNamespace(param_groups=[{"params": params[:30]}, {"params": params[30:]}])
        found = cls("cuda")._unscale_grads_(opt, torch.full((), inv, device=cuda), torch.zeros((), device=cuda),
                                            case.startswith("fp16"))
        outs.append(([p.grad for p in params if p.grad is not None], found))
    (ga, fa), (gb, fb) = outs
    assert len(ga) == len(gb) == N_TENSORS - 1 + case.startswith("fp16")
    for a, b in zip(ga, gb):
        assert torch.equal(_bits(a), _bits(b))
    assert fa.keys() == fb.keys() and len(fa) == 1
    for d in fa:
        assert float(fa[d]) == float(fb[d]) == float(case not in ("clean", "fp16_member"))


def test_grad_scaler_refuses_fp16_unscale(cuda):
    import types
    h = torch.zeros(3, device=cuda, dtype=torch.float16).requires_grad_(True)
    h.grad = torch.zeros(3, device=cuda, dtype=torch.float16)
    opt = types.SimpleNamespace(param_groups=[{"params": [h]}])
    with pytest.raises(ValueError, match="FP16"):
        _dgx("GradScaler")("cuda")._unscale_grads_(opt, torch.ones((), device=cuda), torch.zeros((), device=cuda),
                                                   False)


def test_grad_scaler_full_loop(cuda):
    """scale(loss).backward(); step; update on a two-layer net with dgx.optim.AdamW:
    dgx.optim.GradScaler == torch.amp.GradScaler, parameters bit-equal and the
    scale equal (growth_interval 2: the scale moves within the three iterations)."""
    torch.manual_seed(5)
    x, y = torch.randn(32, 16, device=cuda), torch.randn(32, 4, device=cuda)
    proto = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4)).to(cuda)
    ends = []
    for cls in (_dgx("GradScaler"), torch.amp.GradScaler):
        net = torch.nn.Sequential(torch.nn.Linear(16, 32), torch.nn.ReLU(), torch.nn.Linear(32, 4)).to(cuda)
        net.load_state_dict(proto.state_dict())
        opt = _dgx("AdamW")(net.parameters(), lr=1e-2, weight_decay=1e-4)
        sc = cls("cuda", init_scale=SCALE, growth_interval=2)
        for _ in range(3):
            opt.zero_grad()
            loss = torch.nn.functional.mse_loss(net(x), y)
            sc.scale(loss).backward()
            sc.step(opt)
            sc.update()
        ends.append(([p.detach().clone() for p in net.parameters()], sc.get_scale()))
    (pa, sa), (pb, sb) = ends
    assert sa == sb == 2 * SCALE
    for a, b, p0 in zip(pa, pb, proto.parameters()):
        assert torch.equal(a, b) and not torch.equal(a, p0.detach())


# ---- 6. state dicts ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direction", ["torch_to_dgx", "dgx_to_torch"])
def test_adam_state_dict_round_trip(cuda, direction):
    """Three steps with one class, load_state_dict into the other kind, two more
    steps on each: equal within the bar of test 1 (amsgrad, so all four keys)."""
    kw = ADAM_SETTINGS["amsgrad"][1]
    spread = _torch_adam(cuda, "amsgrad")[2]

    def theirs(ps):
        return torch.optim.Adam(ps, foreach=False, fused=False, **kw)

    def ours(ps):
        return _dgx("Adam")(ps, **kw)
    first, second = (theirs, ours) if direction == "torch_to_dgx" else (ours, theirs)
    _, opt_a, params_a = _run(first, cuda)
    params_b = _params(cuda)
    with torch.no_grad():
        for b, a in zip(params_b, params_a):
            b.copy_(a)
    opt_b = second(params_b)
    opt_b.load_state_dict(copy.deepcopy(opt_a.state_dict()))   # load_state_dict shares tensors it need not cast
    recs = []
    for opt, params in ((opt_a, params_a), (opt_b, params_b)):
        rec = []
        for s in range(3, 5):
            _set_grads(params, s, cuda)
            before = [p.detach().clone() for p in params]
            opt.step()
            snap = _snapshot(opt, params)
            snap["upd"] = [x - y for x, y in zip(snap["p"], before)]
            rec.append(snap)
        recs.append(rec)
    ref, got = (recs[0], recs[1]) if direction == "torch_to_dgx" else (recs[1], recs[0])
    _assert_within(_distance(got, ref), spread, "state dict " + direction)
    dgx_opt, dgx_params = (opt_b, params_b) if direction == "torch_to_dgx" else (opt_a, params_a)
    st = dgx_opt.state[dgx_params[0]]["step"]
    assert st.is_cuda and st.dtype == torch.float32 and float(st) == 5
