"""Host side of the Adam / RMSprop optimizers and the ``train.amp`` loss scaler (no GPU): ``get_optimizer``'s name -> class
mapping, groups and ``lr_names`` (reference optim.py:54-124), the Trainer's refusal of ExtraAdam under ``train.amp``
(trainer.py:116-126), the scaler's host rule against the fixture's recorded trajectory (tests/golden/amp_optim.npz, written
by tests/devtools/make_golden_amp_optim.py from the reference's optimizers + ``torch.amp.GradScaler("cpu")``) and against a
live ``torch.amp.GradScaler("cpu")``, the C ABI's argument validation, and ``load_state_dict`` with int / tensor ``step``."""
import ctypes
import json

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_golden


@pytest.fixture(scope="module")
def lib():
    from climategan_amd import _lib

    if not _lib.LIB_PATH.exists():
        import __graft_entry__ as g

        g.build()
    return _lib.load()


class _Holder(torch.nn.Module):
    def __init__(self, *shapes):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.zeros(s)) for s in shapes])


def _conf(name, lr):
    from climategan_amd.config import default_opts

    conf = default_opts().dis.opt
    conf.optimizer = name
    conf.lr = lr
    conf.beta1 = 0.5
    return conf


@pytest.mark.parametrize("name, cls", [("Adam", "Adam"), ("adam", "Adam"), ("RMSprop", "RMSprop"), ("rmsprop", "RMSprop"),
                                       ("ExtraAdam", "ExtraAdam"), ("SomethingElse", "Adam")])
def test_get_optimizer_name_to_class(name, cls):
    """optim.py:110-121: extraadam / rmsprop by name, any other name Adam with betas (beta1, 0.999)."""
    from climategan_amd import optim

    net = _Holder((3, 5), (7,))
    opt, sched, names = optim.get_optimizer(net, _conf(name, 3e-4))
    assert type(opt) is getattr(optim, cls) and isinstance(opt, torch.optim.Optimizer)
    assert names == ["full"] and len(opt.param_groups) == 1 and opt.param_groups[0]["lr"] == 3e-4
    assert [tuple(p.shape) for p in opt.param_groups[0]["params"]] == [(3, 5), (7,)]
    if cls == "Adam":       # torch.optim.Adam's defaults, the reference's betas
        g = opt.param_groups[0]
        assert (g["betas"], g["eps"], g["weight_decay"], g["amsgrad"]) == ((0.5, 0.999), 1e-8, 0, False)
    if cls == "RMSprop":    # torch.optim.RMSprop's defaults (the reference passes the learning rate only)
        g = opt.param_groups[0]
        assert (g["alpha"], g["eps"], g["weight_decay"], g["momentum"], g["centered"]) == (0.99, 1e-8, 0, 0, False)


@pytest.mark.parametrize("name", ["Adam", "RMSprop"])
def test_get_optimizer_groups_and_lr_names(name):
    """Per-task groups of a discriminator (optim.py:82-108): same groups, order, rates and lr_names as for ExtraAdam."""
    from climategan_amd.optim import get_optimizer

    net = torch.nn.ModuleDict({"m": _Holder((2, 3)), "s": _Holder((4,), (5, 1)), "p": _Holder((6,))})
    lr = {"default": 1e-4, "m": 2e-4, "s": 3e-4}
    opt, _, names = get_optimizer(net, _conf(name, lr), ["m", "s", "d", "p"], True)
    ext, _, ext_names = get_optimizer(net, _conf("ExtraAdam", lr), ["m", "s", "d", "p"], True)
    assert names == ext_names == ["disc_m", "disc_s", "disc_p"]
    assert [g["lr"] for g in opt.param_groups] == [g["lr"] for g in ext.param_groups] == [2e-4, 3e-4, 1e-4]
    assert [[id(p) for p in g["params"]] for g in opt.param_groups] == [[id(p) for p in g["params"]] for g in ext.param_groups]


@pytest.mark.parametrize("name", ["RAdam", "novograd"])
def test_get_optimizer_refuses_torch_optimizer_names(name):
    from climategan_amd.optim import get_optimizer

    with pytest.raises(NotImplementedError, match="torch_optimizer.*cannot be pinned"):
        get_optimizer(_Holder((3,)), _conf(name, 1e-4))


def test_unsupported_variants_are_refused():
    from climategan_amd.optim import Adam, RMSprop

    ps = [torch.nn.Parameter(torch.zeros(3))]
    with pytest.raises(NotImplementedError, match="amsgrad"):
        Adam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError, match="momentum"):
        RMSprop(ps, momentum=0.9)
    with pytest.raises(NotImplementedError, match="centered"):
        RMSprop(ps, centered=True)
    with pytest.raises(ValueError, match="beta parameter at index 0"):
        Adam(ps, betas=(1.0, 0.999))
    ps[0].grad = torch.zeros(3)
    with pytest.raises(RuntimeError, match="contiguous fp32 device parameters"):
        Adam(ps).step()                       # a host tensor: there is no CPU fallback


def test_trainer_refuses_extra_adam_under_amp():
    """reference trainer.py:116-126."""
    from climategan_amd.config import default_opts
    from climategan_amd.optim import GradScaler
    from climategan_amd.trainer import Trainer

    opts = default_opts()
    assert opts.train.amp is False
    assert Trainer(opts, device="cpu").grad_scaler_g is None
    opts.train.amp = True
    with pytest.raises(ValueError, match="AMP does not work with ExtraAdam"):
        Trainer(opts, device="cpu")
    opts.gen.opt.optimizer = "Adam"
    with pytest.raises(ValueError, match="AMP does not work with ExtraAdam"):
        Trainer(opts, device="cpu")           # the discriminators' optimizer still is
    opts.dis.opt.optimizer = "adam"
    T = Trainer(opts, device="cpu")
    assert isinstance(T.grad_scaler_g, GradScaler) and isinstance(T.grad_scaler_d, GradScaler)
    assert T.grad_scaler_g is not T.grad_scaler_d and T.grad_scaler_g.get_scale() == 65536.0


@pytest.mark.parametrize("which", ["adam", "rmsprop"])
def test_scaler_rule_replays_the_fixture(which):
    from climategan_amd.optim import GradScaler

    case = json.loads((GOLDEN / "amp_optim_case.json").read_text())["amp_optim"]
    gold = load_golden("amp_optim")
    found = gold[which + ".found"]
    assert found.tolist() == [int(i + 1 in (case["inf_at"]["step"], case["nan_at"]["step"])) for i in range(case["steps"])]
    s = GradScaler(init_scale=case["init_scale"], growth_interval=case["growth_interval"])
    for i, f in enumerate(found):
        s.advance(bool(f))
        assert s.get_scale() == gold[which + ".scales"][i] and s.get_growth_tracker() == gold[which + ".trackers"][i], i
    assert s.skipped_steps == 2
    assert s.get_scale() == case["init_scale"] / 2            # halved twice, doubled once after three clean steps


def test_scaler_rule_matches_live_torch_gradscaler():
    from climategan_amd.optim import GradScaler

    kw = dict(init_scale=1024.0, growth_factor=4.0, backoff_factor=0.25, growth_interval=2)
    ref = torch.amp.GradScaler("cpu", **kw)
    mine = GradScaler(**kw)
    p = torch.nn.Parameter(torch.zeros(2))
    opt = torch.optim.SGD([p], lr=0.1)
    for i, bad in enumerate([0, 0, 0, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 0]):
        ref.scale(torch.zeros(()))
        p.grad = torch.tensor([1.0, float("nan") if bad and i % 2 else float("-inf") if bad else 2.0])
        ref.step(opt)
        ref.update()
        mine.advance(bool(bad))
        assert mine.get_scale() == ref.get_scale() and mine.get_growth_tracker() == ref._get_growth_tracker(), i
    sd = mine.state_dict()
    assert sd == {k: (v if not torch.is_tensor(v) else v.item()) for k, v in ref.state_dict().items()}
    other = GradScaler()
    other.load_state_dict(sd)
    assert other.state_dict() == sd
    off = GradScaler(enabled=False)
    assert off.get_scale() == 1.0 and off.state_dict() == {}


def test_entry_points_validate_on_the_host(lib):
    """Null tables, a zero count and bad hyper-parameters: error code + message before any launch."""
    table = ctypes.addressof(ctypes.create_string_buffer(64))       # never dereferenced: validation comes first
    flag = ctypes.addressof(ctypes.create_string_buffer(4))
    adam_ok = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0)
    for args in ((None, 1, 8) + adam_ok, (table, 0, 8) + adam_ok, (table, 1, 0) + adam_ok):
        assert lib.cgan_adam_multi_tensor(*args, None, None) != 0
        assert b"adam: bad arguments" in lib.cgan_last_error()
    for bad in ((-1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0), (1e-3, 1.0, 0.999, 1e-8, 0.0, 1.0), (1e-3, 0.9, -0.1, 1e-8, 0.0, 1.0),
                (1e-3, 0.9, 0.999, -1e-8, 0.0, 1.0), (1e-3, 0.9, 0.999, 1e-8, -0.5, 1.0)):
        assert lib.cgan_adam_multi_tensor(table, 1, 8, *bad, None, None) != 0
        assert b"adam: Invalid hyper-parameter" in lib.cgan_last_error()
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.cgan_adam_multi_tensor(table, 1, 8, 1e-3, 0.9, 0.999, 1e-8, 0.0, inv, None, None) != 0
        assert b"inv_scale" in lib.cgan_last_error()
    assert lib.cgan_rmsprop_multi_tensor(None, 1, 8, 1e-2, 0.99, 1e-8, 0.0, 1.0, None, None) != 0
    assert b"rmsprop: bad arguments" in lib.cgan_last_error()
    assert lib.cgan_rmsprop_multi_tensor(table, 1, 8, 1e-2, -0.99, 1e-8, 0.0, 1.0, None, None) != 0
    assert b"rmsprop: Invalid hyper-parameter" in lib.cgan_last_error()
    assert lib.cgan_grads_nonfinite_check_multi_tensor(None, 1, 8, 1.0, 0, flag, None) != 0
    assert lib.cgan_grads_nonfinite_check_multi_tensor(table, 0, 8, 1.0, 0, flag, None) != 0
    assert b"grads_nonfinite_check: bad arguments" in lib.cgan_last_error()
    assert lib.cgan_grads_nonfinite_check_multi_tensor(table, 1, 8, 1.0, 0, None, None) != 0
    assert b"found_inf_device is null" in lib.cgan_last_error()
    assert lib.cgan_grads_nonfinite_check_multi_tensor(table, 1, 8, 1.0, 2, flag, None) != 0
    assert b"write_back" in lib.cgan_last_error()
    assert lib.cgan_grads_nonfinite_check_multi_tensor(table, 1, 8, 0.0, 1, flag, None) != 0
    assert b"inv_scale" in lib.cgan_last_error()
    assert lib.cgan_amp_optim_finish(None, 1, None, None) != 0
    assert lib.cgan_amp_optim_finish(table, 0, None, None) != 0
    assert b"amp_optim_finish: bad arguments" in lib.cgan_last_error()


@pytest.mark.parametrize("cls, keys", [("Adam", ("exp_avg", "exp_avg_sq")), ("RMSprop", ("square_avg",))])
def test_load_state_dict_accepts_int_and_tensor_step(cls, keys):
    """Old torch (the reference's checkpoints) stores ``step`` as an int, current torch as a tensor: both end up in the
    optimizer's own fp32 scalars on the parameter's device; ``state_dict()`` round-trips."""
    from climategan_amd import optim

    def make():
        return getattr(optim, cls)([torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(2, 3))], lr=1e-3)

    g = torch.Generator().manual_seed(3)
    for step in (7, 7.0, torch.tensor(7.0), torch.tensor(7)):
        opt = make()
        state = {i: dict({"step": step.clone() if torch.is_tensor(step) else step},
                         **{k: torch.rand(s, generator=g) for k in keys}) for i, s in enumerate([(5,), (2, 3)])}
        sd = {"state": state, "param_groups": opt.state_dict()["param_groups"]}
        opt.load_state_dict(sd)
        for i, p in enumerate(opt.param_groups[0]["params"]):
            st = opt.state[p]
            assert torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32 and st["step"].dim() == 0
            assert st["step"].device == p.device and st["step"].item() == 7.0
            for k in keys:
                assert torch.equal(st[k], state[i][k])
        assert opt.state[opt.param_groups[0]["params"][0]]["step"].data_ptr() != \
            opt.state[opt.param_groups[0]["params"][1]]["step"].data_ptr()
        again = make()
        again.load_state_dict(opt.state_dict())
        a, b = opt.state_dict(), again.state_dict()
        assert a["param_groups"] == b["param_groups"] and a["state"].keys() == b["state"].keys()
        for i in a["state"]:
            for k in a["state"][i]:
                assert np.array_equal(a["state"][i][k].numpy(), b["state"][i][k].numpy()), (i, k)
