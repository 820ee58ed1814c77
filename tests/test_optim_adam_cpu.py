"""dgx.optim.Adam / AdamW / GradScaler host logic (no GPU): torch's argument
checks and defaults, the GradScaler protocol flag on all three optimizers, a
loud refusal of parameters the HIP kernels cannot take (no silent CPU path),
and a disabled scaler passing through."""
import pytest
import torch


def _param():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
@pytest.mark.parametrize("kw", [dict(lr=-1.0), dict(eps=-1e-8), dict(weight_decay=-1e-4), dict(betas=(-0.1, 0.999)),
                                dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)), dict(betas=(0.9, -0.5))])
def test_adam_argument_checks_equal_torch(name, kw):
    import dgx.optim
    with pytest.raises(ValueError) as ours:
        getattr(dgx.optim, name)(_param(), **kw)
    with pytest.raises(ValueError) as theirs:
        getattr(torch.optim, name)(_param(), **kw)
    assert str(ours.value) == str(theirs.value)


def test_adam_defaults_equal_torch():
    from dgx.optim import Adam, AdamW
    for ours, theirs in ((Adam, torch.optim.Adam), (AdamW, torch.optim.AdamW)):
        a, b = ours(_param()).defaults, theirs(_param()).defaults
        assert a == b, (a, b)
    assert AdamW(_param()).defaults["weight_decay"] == 0.01
    assert AdamW(_param()).defaults["decoupled_weight_decay"] is True
    assert Adam(_param()).defaults["decoupled_weight_decay"] is False
    assert Adam(_param(), decoupled_weight_decay=True).defaults["decoupled_weight_decay"] is True
    opt = Adam(_param(), lr=1e-2, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-4, amsgrad=True, maximize=True)
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["amsgrad"], g["maximize"]) == \
        (1e-2, (0.8, 0.9), 1e-6, 1e-4, True, True)


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_adam_implementation_switches(name):
    """torch's foreach / fused / capturable / differentiable choose between its
    implementations; there is one here, so they pass only when unset."""
    import dgx.optim
    cls = getattr(dgx.optim, name)
    cls(_param(), foreach=None, fused=None, capturable=False, differentiable=False)
    cls(_param(), foreach=False, fused=False)
    for kw in (dict(foreach=True), dict(fused=True), dict(capturable=True), dict(differentiable=True)):
        with pytest.raises(ValueError):
            cls(_param(), **kw)


def test_step_supports_amp_scaling():
    from dgx.optim import SGD, Adam, AdamW
    for opt in (SGD(_param(), lr=0.1), Adam(_param()), AdamW(_param())):
        assert opt._step_supports_amp_scaling is True


@pytest.mark.parametrize("name", ["Adam", "AdamW"])
def test_adam_refuses_host_parameters(name):
    import dgx.optim
    cls = getattr(dgx.optim, name)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    opt = cls([p], lr=0.1)
    with pytest.raises(TypeError):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(3)) and len(opt.state) == 0
    q = torch.nn.Parameter(torch.zeros(3))   # no gradient: skipped, nothing launched
    opt = cls([q], lr=0.1)
    opt.step()
    assert len(opt.state) == 0


def test_adam_refuses_other_dtypes():
    from dgx.optim import Adam
    p = torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))
    p.grad = torch.ones(3, dtype=torch.float64)
    with pytest.raises(TypeError):
        Adam([p]).step()


def test_disabled_grad_scaler_passes_through():
    from dgx.optim import GradScaler

    class Counting(torch.optim.SGD):
        calls = 0

        def step(self, closure=None):
            type(self).calls += 1
            return "stepped"

    scaler = GradScaler("cuda", enabled=False)
    assert isinstance(scaler, torch.amp.GradScaler) and not scaler.is_enabled()
    loss = torch.ones(())
    assert scaler.scale(loss) is loss
    opt = Counting(_param(), lr=0.1)
    assert scaler.step(opt) == "stepped" and Counting.calls == 1
    scaler.update()
    scaler.unscale_(opt)
