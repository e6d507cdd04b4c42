"""vitmi.optim.Adam's weight average without a GPU: constructor validation, storage and state keys
(a parameter list of CPU tensors; nothing here launches)."""
import pytest
import torch

from vitmi import optim


def params():
    g = torch.Generator().manual_seed(0)
    return [torch.randn(n, generator=g).requires_grad_(True) for n in (5, 64, 1027)]


def test_defaults_are_keras():
    opt = optim.Adam(params())
    assert opt.use_ema is False and opt.ema_momentum == 0.99 and opt.ema_overwrite_frequency is None


@pytest.mark.parametrize("bad", [1.0, 1.5, -0.1, float("nan")])
def test_momentum_outside_the_range_is_refused_at_construction(bad):
    with pytest.raises(ValueError):
        optim.Adam(params(), use_ema=True, ema_momentum=bad)


def test_a_callable_momentum_is_checked_at_the_step():
    opt = optim.Adam(params(), use_ema=True, ema_momentum=lambda t: 2.0)      # constructing is fine
    for p in opt.params:
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError):
        opt.step()


@pytest.mark.parametrize("bad", [0, -1, 1.5, True])
def test_overwrite_frequency_is_an_int_from_one(bad):
    with pytest.raises(ValueError):
        optim.Adam(params(), use_ema=True, ema_overwrite_frequency=bad)
    assert optim.Adam(params(), use_ema=True, ema_overwrite_frequency=1).ema_overwrite_frequency == 1


def test_without_use_ema_there_is_no_average():
    opt = optim.Adam(params())
    assert opt._ema is None
    assert set(opt.state_dict()) == {"iterations", "learning_rate", "m", "v"}
    for call in (opt.swap_ema, opt.finalize_variable_values, opt.reset_ema, opt.ema_parameters):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        with opt.ema_weights():
            pass


def test_list_path_average_starts_as_copies_not_aliases():
    ps = params()
    opt = optim.Adam(ps, use_ema=True)
    avg = opt.ema_parameters()
    assert isinstance(avg, list) and len(avg) == 3
    for p, e in zip(ps, avg):
        assert torch.equal(p.detach(), e) and e.data_ptr() != p.data_ptr() and not e.requires_grad
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(avg, opt.ema_parameters()))     # views, not copies
    with torch.no_grad():
        ps[0].add_(1.0)
    assert not torch.equal(ps[0].detach(), avg[0])
    opt.reset_ema()
    assert torch.equal(ps[0].detach(), avg[0])


def test_state_dict_carries_the_average():
    ps = params()
    opt = optim.Adam(ps, use_ema=True)
    sd = opt.state_dict()
    assert set(sd) == {"iterations", "learning_rate", "m", "v", "ema"}
    assert all(torch.equal(a, b) and a.data_ptr() != b.data_ptr() for a, b in zip(sd["ema"], opt.ema_parameters()))
    # loading: "ema" is copied when present; absent, the average restarts from the parameters
    sd["ema"] = [torch.full_like(e, 7.0) for e in sd["ema"]]
    opt.load_state_dict(sd)
    assert all(bool((e == 7.0).all()) for e in opt.ema_parameters())
    del sd["ema"]
    opt.load_state_dict(sd)
    assert all(torch.equal(p.detach(), e) for p, e in zip(ps, opt.ema_parameters()))
    # a state with an average loads into an optimizer without one
    plain = optim.Adam(ps)
    plain.load_state_dict(opt.state_dict())
    assert plain._ema is None
