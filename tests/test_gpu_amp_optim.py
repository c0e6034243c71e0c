"""GPU tests of the fused Adam / RMSprop updates and the ``train.amp`` loss-scaling path (csrc/amp_optim.hip,
climategan_amd.optim.Adam / RMSprop / GradScaler, Trainer with ``train.amp``).

What is pinned, and against what:
  * the optimizer and scaler arithmetic against torch -- the trajectory of ``torch.optim.Adam`` / ``RMSprop`` as the
    reference's ``get_optimizer`` builds them, driven with ``torch.amp.GradScaler("cpu")`` (tests/golden/amp_optim.npz,
    tests/devtools/make_golden_amp_optim.py), and a live ``torch.optim.Adam`` on the GPU.  fp32 element-wise arithmetic:
    2e-6 relative, the figure of tests/test_gpu_optim.py for the same arithmetic class (torch and the kernel contract
    multiply-adds differently);
  * the AMP train step against the already tested static-scale fp16 step, bit for bit: 1/64 is exact in fp32, so
    unscaling in the update's registers and unscaling in a pass over the gradients give the same numbers.
The reference's own fp16 autocast forward needs CUDA: there is no reference-side golden for the values of an AMP step.
"""
import json

import numpy as np
import pytest
import torch

from helpers import GOLDEN, case_state_dict, golden_cases, gstep_d_state_dict, load_golden, t
from oracle.make_golden import case_inputs

pytestmark = pytest.mark.gpu
GNAME, MNAME = "gstep_p", "mstep"
RTOL = 2e-6


def close(got, ref, floor=0.0):
    got, ref = got.detach().cpu().numpy().astype(np.float64), np.asarray(ref, dtype=np.float64)
    err, bound = np.abs(got - ref).max(), RTOL * max(floor, np.abs(ref).max())
    return err <= bound, (err, bound)


# ------------------------------------------------------------------------------------------------ optimizer + scaler
@pytest.mark.parametrize("which", ["adam", "rmsprop"])
def test_trajectory_matches_the_reference_fixture(which):
    from climategan_amd import optim

    case = json.loads((GOLDEN / "amp_optim_case.json").read_text())["amp_optim"]
    gold = {k[len(which) + 1:]: v for k, v in load_golden("amp_optim").items() if k.startswith(which + ".")}
    n = len(case["shapes"])
    params = [torch.nn.Parameter(t(gold["p%d_init" % i]).cuda()) for i in range(n)]
    groups = [{"params": [params[i] for i in idx], "lr": lr, "weight_decay": wd}
              for idx, lr, wd in zip(case["groups"], case["lr"], case["weight_decay"])]
    opt = optim.Adam(groups, betas=(case["beta1"], 0.999)) if which == "adam" else optim.RMSprop(groups)
    mkeys = [("exp_avg", "m"), ("exp_avg_sq", "v")] if which == "adam" else [("square_avg", "v")]
    scaler = optim.GradScaler(init_scale=case["init_scale"], growth_interval=case["growth_interval"])
    skipped = []
    for it in range(1, case["steps"] + 1):
        scale = scaler.get_scale()
        assert scale == (gold["scales"][it - 2] if it > 1 else case["init_scale"])
        for i, p in enumerate(params):
            p.grad = t(gold["g%d_%d" % (i, it)]).cuda() * scale
        for what, value in (("inf_at", float("inf")), ("nan_at", float("nan"))):
            if case[what]["step"] == it:
                params[case[what]["tensor"]].grad.view(-1)[case[what]["index"]] = value
        grads = [p.grad.clone() for p in params]
        before = [(p.detach().clone(), {k: v.clone() for k, v in opt.state[p].items()}) for p in params]
        scaler.step(opt)
        scaler.update()
        for i, p in enumerate(params):
            assert torch.equal(p.grad, grads[i]) or it in (case["inf_at"]["step"], case["nan_at"]["step"])   # left scaled
            st = opt.state[p]
            if gold["found"][it - 1]:
                # a skipped step: every p, m, v of every tensor bit-identical, no step advanced
                assert torch.equal(p.detach(), before[i][0]), (it, i)
                for k, v in before[i][1].items():
                    assert torch.equal(st[k], v), (it, i, k)
            ok, stat = close(p, gold["p%d_after%d" % (i, it)], 1.0)
            assert ok, ("p", it, i, stat)
            for key, gk in mkeys:
                ok, stat = close(st[key], gold["%s%d_after%d" % (gk, i, it)])
                assert ok, (key, it, i, stat)
            assert st["step"].item() == gold["steps"][it - 1][i], (it, i)
        new_scale = scaler.get_scale()
        assert new_scale == gold["scales"][it - 1] and scaler.get_growth_tracker() == gold["trackers"][it - 1], it
        if gold["found"][it - 1]:
            assert new_scale == scale / 2
            skipped.append(it)
    assert skipped == [case["inf_at"]["step"], case["nan_at"]["step"]] and scaler.skipped_steps == 2
    assert gold["found"][-3:].tolist() == [0, 0, 0] and scaler.get_scale() == 2 * gold["scales"][-2]   # three clean steps


def test_adam_matches_live_torch_adam_on_the_gpu():
    from climategan_amd.optim import Adam

    g = torch.Generator().manual_seed(0)
    odd = torch.randn(1000, generator=g).cuda()           # a tensor that does not start on a 16-byte boundary
    ps = [torch.randn(300_001, generator=g).cuda(), torch.randn(17, generator=g).cuda(), torch.randn(17, generator=g).cuda(),
          odd[1:]]
    mine = [torch.nn.Parameter(p.clone()) for p in ps[:3]] + [torch.nn.Parameter(odd.clone()[1:])]
    assert mine[3].data_ptr() % 16 == 4
    theirs = [torch.nn.Parameter(p.clone()) for p in ps]
    kw = dict(lr=2e-5, betas=(0.5, 0.999), weight_decay=0.01)
    opt, ref = Adam(mine, **kw), torch.optim.Adam(theirs, **kw)
    for st in range(3):
        grads = [torch.randn(p.shape, generator=g).cuda() for p in ps]
        grads[2] = None                                    # e.g. spectral-norm u / v (requires_grad=False)
        for a, b, gr in zip(mine, theirs, grads):
            a.grad = gr
            b.grad = None if gr is None else gr.clone()
        opt.step()
        ref.step()
        for i, (a, b) in enumerate(zip(mine, theirs)):
            ok, stat = close(a, b.detach().cpu().numpy(), 1.0)
            assert ok, (st, i, stat)
    for i in (0, 1, 3):
        for key in ("exp_avg", "exp_avg_sq"):
            ok, stat = close(opt.state[mine[i]][key], ref.state[theirs[i]][key].cpu().numpy())
            assert ok, (i, key, stat)
        assert opt.state[mine[i]]["step"].item() == 3
    assert torch.equal(mine[2].detach(), ps[2])           # no gradient: untouched, its step stays at 0
    assert float(opt.state[mine[2]].get("step", 0)) == 0


def test_nonfinite_values_are_found_anywhere_in_the_largest_tensor():
    """-inf, +inf and NaN at the first, a middle and the last element of the largest tensor (the grid-stride tail
    included); finite values near fp32's maximum are not flagged."""
    from climategan_amd.optim import Adam

    n = 300_001 + 4096 * 1024                              # more than one grid-stride round of 1024 blocks x 1024 elements
    params = [torch.nn.Parameter(torch.zeros(1000, device="cuda")), torch.nn.Parameter(torch.zeros(n, device="cuda"))]
    opt = Adam(params, lr=1e-3)
    flag = torch.zeros(1, device="cuda")
    params[0].grad = torch.ones(1000, device="cuda")
    for value in (float("-inf"), float("inf"), float("nan")):
        for index in (0, n // 2 + 1, n - 1):
            params[1].grad = torch.ones(n, device="cuda")
            params[1].grad[index] = value
            flag.zero_()
            opt.step(inv_scale=1.0 / 1024, found_inf=flag, check=True)
            assert flag.item() == 1.0, (value, index)
            assert not params[0].any() and not params[1].any()                  # skipped: nothing written
            assert all(opt.state[p]["step"].item() == 0 for p in params)
    big = torch.finfo(torch.float32).max
    params[1].grad = torch.full((n,), big, device="cuda")
    params[1].grad[::2] = -big
    params[1].grad[n - 1] = big
    flag.zero_()
    opt.step(inv_scale=2.0 ** -120, found_inf=flag, check=True)
    assert flag.item() == 0.0
    assert all(opt.state[p]["step"].item() == 1 for p in params)
    assert torch.isfinite(params[1]).all() and params[1].abs().min() > 0


def test_unscale_writes_the_unscaled_gradients_and_sets_the_flag():
    from climategan_amd.optim import Adam, GradScaler

    g = torch.Generator().manual_seed(1)
    true = [torch.randn(70_003, generator=g).cuda(), torch.randn(5, generator=g).cuda()]
    params = [torch.nn.Parameter(torch.zeros_like(x)) for x in true]
    opt = Adam(params, lr=1e-3)
    ref_p = [torch.nn.Parameter(torch.zeros_like(x)) for x in true]
    ref = torch.optim.Adam(ref_p, lr=1e-3)
    scaler = GradScaler(init_scale=4096.0, growth_interval=100)
    for p, x in zip(params, true):
        p.grad = x * 4096.0
    scaler.unscale_(opt)
    for p, x in zip(params, true):
        assert torch.equal(p.grad, x)                      # g / scale, exact for a power of two
    with pytest.raises(RuntimeError, match="already been called"):
        scaler.unscale_(opt)
    scaler.step(opt)                                       # must not unscale a second time
    scaler.update()
    for p, x in zip(ref_p, true):
        p.grad = x.clone()
    ref.step()
    for a, b in zip(params, ref_p):
        ok, stat = close(a, b.detach().cpu().numpy(), 1.0)
        assert ok, stat
    assert scaler.get_scale() == 4096.0 and scaler.get_growth_tracker() == 1
    # a non-finite value: found by unscale_'s own check, the step is skipped, the scale halves
    keep = [p.detach().clone() for p in params]
    for p, x in zip(params, true):
        p.grad = x * 4096.0
    params[0].grad[-1] = float("-inf")
    scaler.unscale_(opt)
    assert torch.equal(params[0].grad[:-1], true[0][:-1]) and params[0].grad[-1].item() == float("-inf")
    scaler.step(opt)
    scaler.update()
    assert all(torch.equal(p.detach(), k) for p, k in zip(params, keep))
    assert scaler.get_scale() == 2048.0 and scaler.get_growth_tracker() == 0
    assert all(opt.state[p]["step"].item() == 1 for p in params)
    with pytest.raises(RuntimeError, match="No inf checks"):
        scaler.update()


# ------------------------------------------------------------------------------------------------ Trainer
def painter_opts(case, amp):
    from climategan_amd.config import default_opts

    opts = default_opts()
    opts.tasks = ["p"]
    opts.gen.p.latent_dim = case["latent_dim"]
    opts.gen.p.spade_n_up = case["n_up"]
    opts.dis.p.ndf, opts.dis.p.n_layers, opts.dis.p.num_D = case["ndf"], case["n_layers"], case["num_D"]
    opts.dis.soft_shift, opts.dis.flip_prob = 0.0, 0.0
    opts.train.lambdas.G.p.vgg = 0
    opts.gen.opt.optimizer = opts.dis.opt.optimizer = "Adam"
    opts.gen.opt.lr_policy = opts.dis.opt.lr_policy = "constant"
    opts.train.amp = amp
    return opts


def painter_trainer(case, amp, opts=None):
    from climategan_amd.optim import Adam
    from climategan_amd.trainer import Trainer

    T = Trainer(opts if opts is not None else painter_opts(case, amp), device="cuda").setup(inference=False)
    assert type(T.g_opt) is Adam and type(T.d_opt) is Adam
    T.G.painter.load_state_dict(case_state_dict(case), strict=True)
    T.D["p"].load_state_dict(gstep_d_state_dict(case), strict=True)
    T.G.painter.set_latent_shape((case["B"], 3, case["H"], case["W"]), True)
    return T


def d_dtypes(D):
    return {m.compute_dtype for m in D.modules() if hasattr(m, "compute_dtype")}


def painter_batch(case):
    inp = {k: t(v).cuda() for k, v in case_inputs(GNAME, case).items()}
    return {"rf": {"data": {"x": inp["x"], "m": inp["m"]}}}


def test_amp_step_equals_the_static_scale_fp16_step_bit_for_bit():
    from climategan_amd import autograd as ag
    from climategan_amd.optim import GradScaler

    case = golden_cases()[GNAME]
    batch = painter_batch(case)
    torch.manual_seed(5)
    A = painter_trainer(case, True)
    assert A.G.compute_dtype == torch.float16 and d_dtypes(A.D) == {torch.float16}
    A.grad_scaler_g = GradScaler(init_scale=64.0, growth_interval=10 ** 9)
    A.grad_scaler_d = GradScaler(init_scale=64.0, growth_interval=10 ** 9)
    for _ in range(2):
        A.train_step(batch)
    assert ag.GRAD_SCALE == 1.0
    assert A.grad_scaler_g.get_scale() == 64.0 and A.grad_scaler_g.skipped_steps == 0
    assert A.grad_scaler_d.get_scale() == 64.0 and A.grad_scaler_d.skipped_steps == 0

    torch.manual_seed(5)
    B = painter_trainer(case, False)
    # without train.amp the dtype stays bf16
    assert B.grad_scaler_g is None and B.G.compute_dtype == torch.bfloat16 and d_dtypes(B.D) == {torch.bfloat16}
    B.G.set_compute_dtype(torch.float16)
    B.D.set_compute_dtype(torch.float16)
    ag.set_grad_scale(64.0)
    try:
        for _ in range(2):
            B.train_step(batch)
    finally:
        ag.set_grad_scale(1.0)
    diff = []
    for (ka, a), (kb, b) in zip(list(A.G.state_dict().items()) + list(A.D.state_dict().items()),
                                list(B.G.state_dict().items()) + list(B.D.state_dict().items())):
        assert ka == kb
        if not torch.equal(a, b):
            diff.append((ka, (a.float() - b.float()).abs().max().item()))
    print("tensors that differ between the AMP and the static-scale step:", diff)
    assert not diff, diff
    for opt_a, opt_b in ((A.g_opt, B.g_opt), (A.d_opt, B.d_opt)):
        for pa, pb in zip((p for g in opt_a.param_groups for p in g["params"]),
                          (p for g in opt_b.param_groups for p in g["params"])):
            assert opt_a.state[pa].keys() == opt_b.state[pb].keys()
            for k in opt_a.state[pa]:
                assert torch.equal(opt_a.state[pa][k], opt_b.state[pb][k]), k


def test_amp_from_the_default_scale_skips_cleanly_then_trains():
    from climategan_amd import autograd as ag

    case = golden_cases()[GNAME]
    batch = painter_batch(case)
    torch.manual_seed(6)
    T = painter_trainer(case, True)
    assert T.grad_scaler_g.get_scale() == T.grad_scaler_d.get_scale() == 65536.0
    models = (("G", T.G, T.grad_scaler_g), ("D", T.D, T.grad_scaler_d))
    proceeded = {"G": 0, "D": 0}
    log = []
    for it in range(16):
        before = {name: ([p.detach().clone() for p in mod.parameters()], sc.get_scale()) for name, mod, sc in models}
        T.train_step(batch)
        assert ag.GRAD_SCALE == 1.0
        for name, mod, sc in models:
            old, scale0 = before[name]
            same = all(torch.equal(a, p.detach()) for a, p in zip(old, mod.parameters()))
            scale1 = sc.get_scale()
            log.append((it, name, scale0, scale1, same))
            if scale1 < scale0:
                assert same, (it, name)                  # the scale dropped: a skipped step wrote nothing
            else:
                assert not same, (it, name)
                proceeded[name] += 1
            assert all(torch.isfinite(p).all() for p in mod.parameters()), (it, name)
        if min(proceeded.values()) >= 2 and it >= 4:
            break
    print("(iteration, model, scale before, scale after, parameters unchanged):", log)
    assert min(proceeded.values()) >= 2, log             # steps eventually proceed
    assert ag.GRAD_SCALE == 1.0


def test_masker_trainer_with_adam_steps_like_torch_adam():
    """Non-AMP, ``optimizer: Adam`` for G and D on the Masker case: ``step()`` on every iteration (no extrapolation), and
    after the first one every updated parameter equals ``torch.optim.Adam`` applied to a clone with the gradients the
    optimizer saw."""
    from climategan_amd import fill
    from climategan_amd.config import default_opts
    from climategan_amd.optim import Adam
    from climategan_amd.trainer import Trainer

    case = golden_cases()[MNAME]
    opts = default_opts()
    opts.tasks = ["d", "s", "m"]
    opts.gen.opt.optimizer = opts.dis.opt.optimizer = "Adam"
    T = Trainer(opts, device="cuda").setup(inference=False)
    assert type(T.g_opt) is Adam and type(T.d_opt) is Adam and not hasattr(T.g_opt, "extrapolation")
    for mod, seed in ((T.G, case["seed"]), (T.D, case["seed"] + 1)):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in fill.fill_state_dict(shapes, seed, gain=case["gain"]).items()})
    T.G.decoders["d"]._target_size = case["W"] // 4
    T.G.decoders["s"].set_target_size((case["H"] // 4, case["W"] // 4))
    inp = {k: t(v).cuda() for k, v in case_inputs(MNAME, case).items()}
    batch = {dom: {"data": {"x": inp["x_" + dom], "d": inp["d_" + dom], "s": inp["s_" + dom], "m": inp["m_" + dom]}}
             for dom in ("r", "s")}
    calls, seen = {"g": 0, "d": 0}, {}

    def spy(tag, opt):
        inner = opt.step

        def step(*a, **k):
            calls[tag] += 1
            if calls[tag] == 1:
                seen[tag] = [[(p, p.detach().clone(), None if p.grad is None else p.grad.detach().clone())
                              for p in g["params"]] for g in opt.param_groups]
            return inner(*a, **k)
        opt.step = step

    spy("g", T.g_opt)
    spy("d", T.d_opt)
    T.train_step(batch)
    checked = 0
    for tag, opt in (("g", T.g_opt), ("d", T.d_opt)):
        clones = [[torch.nn.Parameter(p0.clone()) for _, p0, _ in grp] for grp in seen[tag]]
        ref = torch.optim.Adam([dict(params=c, lr=g["lr"], betas=g["betas"], eps=g["eps"], weight_decay=g["weight_decay"])
                                for c, g in zip(clones, opt.param_groups)])
        for grp, cl in zip(seen[tag], clones):
            for (_, _, grad), c in zip(grp, cl):
                c.grad = grad
        ref.step()
        for grp, cl in zip(seen[tag], clones):
            for (p, p0, grad), c in zip(grp, cl):
                if grad is None:
                    # not the optimizer's to touch (the spectral-norm u / v move in the forward passes, not here)
                    assert not opt.state[p] and not p.requires_grad
                    continue
                ok, stat = close(p, c.detach().cpu().numpy(), 1.0)
                assert ok, (tag, tuple(p.shape), stat)
                assert not torch.equal(p.detach(), p0) or not grad.any()
                assert opt.state[p]["step"].item() == 1
                checked += 1
    assert checked > 300
    T.train_step(batch)
    assert calls == {"g": 2, "d": 2}                      # step() on the even AND the odd iteration


def test_adam_state_survives_save_and_resume(tmp_path):
    from climategan_amd import fill

    case = golden_cases()[GNAME]
    batch = painter_batch(case)
    opts = painter_opts(case, False)
    opts.output_path = str(tmp_path)
    torch.manual_seed(7)
    A = painter_trainer(case, False, opts)
    for _ in range(2):
        A.train_step(batch)
    A.save()
    B = painter_trainer(case, False, painter_opts(case, False))
    B.opts.output_path = str(tmp_path)
    B.resume()
    assert B.global_step == A.global_step == 2
    pairs = []
    for opt_a, opt_b in ((A.g_opt, B.g_opt), (A.d_opt, B.d_opt)):
        pa = [p for g in opt_a.param_groups for p in g["params"]]
        pb = [p for g in opt_b.param_groups for p in g["params"]]
        assert len(pa) == len(pb)
        for a, b in zip(pa, pb):
            assert torch.equal(a.detach(), b.detach())
            sa, sb = opt_a.state[a], opt_b.state[b]
            assert sa.keys() == sb.keys()
            if sa:
                assert sb["step"].is_cuda and sb["step"].dtype == torch.float32 and sb["step"].item() == sa["step"].item() == 2
                assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"])
                pairs.append((a, b))
    assert len(pairs) > 50
    # one more optimizer step on identical gradients: the resumed run continues exactly like the one that never stopped
    for opt_a, opt_b in ((A.g_opt, B.g_opt), (A.d_opt, B.d_opt)):
        for i, (a, b) in enumerate(zip((p for g in opt_a.param_groups for p in g["params"]),
                                       (p for g in opt_b.param_groups for p in g["params"]))):
            if opt_a.state[a]:
                a.grad = torch.from_numpy(fill.uniform(tuple(a.shape), 1000 + i, -1e-2, 1e-2)).cuda()
                b.grad = a.grad.clone()
            else:
                a.grad = b.grad = None
        opt_a.step()
        opt_b.step()
    for a, b in pairs:
        assert torch.equal(a.detach(), b.detach())
    # ... and one more train step on the same batch.  The fp32 atomics of the bias-gradient and loss reductions differ from
    # run to run and Adam moves a weight whose true gradient is zero by ~lr along the sign of that noise: the bound two
    # runs of the same step are held to in tests/test_gpu_train.py (rtol 1e-3, atol 3e-4 = a few lr)
    torch.manual_seed(8)
    A.train_step(batch)
    torch.manual_seed(8)
    B.train_step(batch)
    for a, b in pairs:
        assert torch.allclose(a.detach(), b.detach(), rtol=1e-3, atol=3e-4)
    for opt in (A.g_opt, B.g_opt, A.d_opt, B.d_opt):
        assert all(st["step"].item() == 4 for st in opt.state.values() if st)
