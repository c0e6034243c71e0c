"""GPU tests of DiffAugment (reference climategan/transforms.py:494-626; kernels climategan_amd/csrc/diffaug.hip).

* The NCHW op and its backward against the reference's recorded runs (tests/golden/diffaug_ops.npz, replaying its draws):
  values within 1e-5, the zero pattern of translation and cutout exactly.
* The fused Painter heads against the NCHW op composed with the paste (same draws): within one 16-bit rounding; the VGG
  half bit for bit ``ops.painter_heads``'.
* A fuzz over shapes and flags against a float64 restatement written here.
* The Painter step with diff_aug fully on (single multi-scale D, and the local / global pair) against the reference's
  (tests/golden/diffaug_step*.npz), with the bounds tests/test_gpu_train.py uses for the same steps; gradients are
  compared on the fixture's seeded sub-sample of each tensor.
* Determinism of a seeded train step with the option on, and the option off / all-off leaving the step unchanged."""
import random

import numpy as np
import pytest
import torch

from helpers import case_state_dict, disc_p_shapes, gstep_d_state_dict, load_golden, t
from oracle.make_golden import case_inputs, grad_subsample

pytestmark = pytest.mark.gpu
SUB = 384
EPS16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}


def _diff_opts(color, tr, cut):
    from climategan_amd.config import default_opts
    o = default_opts().gen.p.diff_aug
    o.update(use=True, do_color_jittering=bool(color), do_translation=tr >= 0, translation_ratio=tr if tr >= 0 else 0.125,
             do_cutout=cut >= 0, cutout_ratio=cut if cut >= 0 else 0.5)
    return o


def _gold_draws(gold, prefix, n):
    return [gold["%sdraw%d" % (prefix, i)] for i in range(n)]


def _op_inputs(name, n, c, h, w):
    from climategan_amd import fill
    return fill.uniform((n, c, h, w), fill.key_seed(name, 1)), fill.uniform((n, c, h, w), fill.key_seed(name, 2))


OPS_GOLD = None


def _ops_gold():
    global OPS_GOLD
    if OPS_GOLD is None:
        OPS_GOLD = load_golden("diffaug_ops")
    return OPS_GOLD


@pytest.mark.parametrize("name", ["all_sq", "all_odd", "all_n1", "color", "color_n1", "translation", "cutout", "cutout_big",
                                  "cutout_zero", "cutout_zero_h"])
def test_nchw_op_and_backward_match_reference(name):
    from climategan_amd.transforms import DiffTransforms, RecordedDraws

    gold = _ops_gold()
    n, c, h, w, color, _ = (int(v) for v in gold[name + ".meta"])
    tr, cut = (float(v) for v in gold[name + ".ratios"])
    src = RecordedDraws(_gold_draws(gold, name + ".", int(gold[name + ".ndraws"][0])))
    x_np, dy_np = _op_inputs(name, n, c, h, w)
    x = t(x_np).cuda().requires_grad_(True)
    y = DiffTransforms(_diff_opts(color, tr, cut), draws=src)(x)
    assert src.used == len(src.values)
    y.backward(t(dy_np).cuda())
    got, ref = y.detach().cpu().numpy(), gold[name + ".y"]
    assert np.abs(got - ref).max() <= 1e-5, (name, np.abs(got - ref).max())
    assert np.array_equal(got == 0, ref == 0), name
    gx, rx = x.grad.cpu().numpy(), gold[name + ".dx"]
    assert np.abs(gx - rx).max() <= 1e-5, (name, np.abs(gx - rx).max())
    if not color:
        assert np.array_equal(gx == 0, rx == 0), name


def test_public_functions_match_the_composed_transform():
    """rand_brightness / contrast / saturation / translation / cutout one at a time, in the reference's order, with the
    same draws = DiffTransforms with everything on."""
    from climategan_amd import transforms as T

    gold = _ops_gold()
    name = "all_odd"
    n, c, h, w, _, _ = (int(v) for v in gold[name + ".meta"])
    tr, cut = (float(v) for v in gold[name + ".ratios"])
    draws = _gold_draws(gold, name + ".", 7)
    x = t(_op_inputs(name, n, c, h, w)[0]).cuda()
    y = T.rand_brightness(x, True, draws=T.RecordedDraws(draws[0:1]))
    y = T.rand_contrast(y, True, draws=T.RecordedDraws(draws[1:2]))
    y = T.rand_saturation(y, True, draws=T.RecordedDraws(draws[2:3]))
    y = T.rand_translation(y, tr, draws=T.RecordedDraws(draws[3:5]))
    y = T.rand_cutout(y, cut, draws=T.RecordedDraws(draws[5:7]))
    assert np.abs(y.cpu().numpy() - gold[name + ".y"]).max() <= 1e-5


def _ref64(x, color, geo, flags, cut_hw):
    """float64 restatement of DiffTransforms (reference transforms.py:494-626) with given draws"""
    from climategan_amd import ops
    n, c, h, w = x.shape
    x = x.double()
    col = color.double().view(n, 3, 1, 1, 1)
    if flags & ops.DA_BRIGHTNESS:
        x = x + (col[:, 0] - 0.5)
    if flags & ops.DA_CONTRAST:
        mean = x.mean(dim=[1, 2, 3], keepdim=True)
        x = (x - mean) * (col[:, 1] + 0.5) + mean
    if flags & ops.DA_SATURATION:
        mean = x.mean(dim=1, keepdim=True)
        x = (x - mean) * (col[:, 2] * 2) + mean
    if flags & ops.DA_TRANSLATION:
        ii = torch.arange(h, device=x.device).view(1, h, 1) + geo[:, 0].view(n, 1, 1)
        jj = torch.arange(w, device=x.device).view(1, 1, w) + geo[:, 1].view(n, 1, 1)
        ok = ((ii >= 0) & (ii < h) & (jj >= 0) & (jj < w)).unsqueeze(1)
        flat = (ii.clamp(0, h - 1) * w + jj.clamp(0, w - 1)).view(n, 1, h * w).expand(n, c, h * w)
        x = torch.gather(x.reshape(n, c, h * w), 2, flat).view(n, c, h, w) * ok
    if flags & ops.DA_CUTOUT and cut_hw[0] > 0 and cut_hw[1] > 0:
        keep = torch.ones(n, h, w, dtype=x.dtype, device=x.device)
        for b in range(n):
            r = (torch.arange(cut_hw[0], device=x.device) + int(geo[b, 2]) - cut_hw[0] // 2).clamp(0, h - 1)
            cc = (torch.arange(cut_hw[1], device=x.device) + int(geo[b, 3]) - cut_hw[1] // 2).clamp(0, w - 1)
            keep[b][r.view(-1, 1), cc.view(1, -1)] = 0
        x = x * keep.unsqueeze(1)
    return x


@pytest.mark.parametrize("seed", range(12))
def test_fuzz_against_float64_restatement(seed):
    from climategan_amd import ops
    from climategan_amd.autograd import DiffAugFn
    from climategan_amd.transforms import draw_params

    g = torch.Generator().manual_seed(1000 + seed)
    n = int(torch.randint(1, 5, (1,), generator=g))
    c = [3, 3, 1, 4][seed % 4]
    h, w = (int(v) for v in torch.randint(1, 70, (2,), generator=g))
    flags_sel = int(torch.randint(1, 32, (1,), generator=g))
    color = tuple(bool(flags_sel & b) for b in (1, 2, 4))
    tr = float(torch.rand(1, generator=g)) * 0.6 if flags_sel & 8 else None
    cut = float(torch.rand(1, generator=g)) * 1.1 if flags_sel & 16 else None
    torch.manual_seed(seed)
    p = draw_params(n, h, w, torch.device("cuda"), color=color, translation_ratio=tr, cutout_ratio=cut)
    x = (torch.rand(n, c, h, w, generator=g) * 2 - 1).cuda().requires_grad_(True)
    dy = (torch.rand(n, c, h, w, generator=g) * 2 - 1).cuda()
    y = DiffAugFn.apply(x, p.color, p.geo, p.flags, p.cut_hw)
    y.backward(dy)
    x64 = x.detach().double().requires_grad_(True)
    y64 = _ref64(x64, p.color, p.geo, p.flags, p.cut_hw)
    y64.backward(dy.double())
    assert (y.detach().double() - y64).abs().max().item() <= 1e-5, (n, c, h, w, p.flags, p.cut_hw)
    if not p.flags & (ops.DA_BRIGHTNESS | ops.DA_CONTRAST | ops.DA_SATURATION):
        assert torch.equal(y.detach() == 0, y64 == 0)
    assert (x.grad.double() - x64.grad).abs().max().item() <= 1e-5, (n, c, h, w, p.flags, p.cut_hw)


def _nhwc_to_nchw3(a):
    return a[..., :3].float().permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("shape", [(3, 40, 56), (1, 33, 17)])
def test_fused_heads_match_the_composed_nchw_op(dt, shape):
    from climategan_amd import fill, ops
    from climategan_amd.transforms import draw_params

    n, h, w = shape
    torch.manual_seed(7)
    fake_t = torch.zeros(n, h, w, 8, dtype=dt, device="cuda")
    fake_t[..., :3] = (torch.rand(n, h, w, 3, device="cuda") * 2 - 1).to(dt)
    x = (torch.rand(n, 3, h, w, device="cuda") * 2 - 1)
    m = t(fill.rect_mask(n, h, w, 5)).cuda()
    m[:, :, : h // 4] = 0.3                                     # a soft band as well
    eps = EPS16[dt]
    for real in (False, True):
        p = draw_params(n, h, w, torch.device("cuda"), color=(True, True, True), translation_ratio=0.2, cutout_ratio=0.5)
        fake = None if real else ops.NHWC(fake_t, 3)
        d_in, v_in = ops.painter_heads_diffaug(fake, x, m, dt, *p, want_vgg=True)
        d0, v0 = ops.painter_heads(fake, x, m, dt, True, True)
        assert torch.equal(v_in.t, v0.t)                                      # the VGG half is untouched
        assert torch.equal(d_in.t[..., 0], d0.t[..., 0])                      # so is the mask channel
        assert torch.equal(d_in.t[..., 4:], torch.zeros_like(d_in.t[..., 4:]))
        pasted = x if real else x * (1 - m) + _nhwc_to_nchw3(fake_t) * m
        ref = ops.diffaug(pasted, *p)
        got = _nhwc_to_nchw3(d_in.t[..., 1:4])
        assert ((got - ref).abs() <= eps * ref.abs() + 1e-6).all(), (got - ref).abs().max().item()
        assert torch.equal(got == 0, ref == 0)
    # backward: d_fake = m * (augment_bwd(d_d_in[1..3]) + 127.5 m d_vgg_in[BGR -> RGB])
    dd = torch.zeros(n, h, w, 8, dtype=dt, device="cuda")
    dd[..., :4] = (torch.rand(n, h, w, 4, device="cuda") * 2 - 1).to(dt)
    dv = torch.zeros(n, h, w, 8, dtype=dt, device="cuda")
    dv[..., :6] = (torch.rand(n, h, w, 6, device="cuda") * 1e-2).to(dt)
    got = _nhwc_to_nchw3(ops.painter_heads_diffaug_bwd(ops.NHWC(dd, 4), ops.NHWC(dv, 6), m, *p).t)
    g = ops.diffaug_bwd(_nhwc_to_nchw3(dd[..., 1:4]), *p) + 127.5 * m * dv[..., [2, 1, 0]].float().permute(0, 3, 1, 2)
    ref = m * g
    assert ((got - ref).abs() <= eps * ref.abs() + 1e-6).all(), (got - ref).abs().max().item()


# ------------------------------------------------------------------------------------------------ train steps
def _step_case(local):
    return dict(kind="gstep_p", latent_dim=32, n_up=4, ndf=16, n_layers=3, num_D=3, H=96, W=128, B=2,
                seed=97 if local else 96)


def _trainer(case, local, dt=torch.float16, diff=True):
    from climategan_amd import fill
    from climategan_amd.config import default_opts
    from climategan_amd.trainer import Trainer

    opts = default_opts()
    opts.tasks = ["p"]
    opts.gen.p.latent_dim, opts.gen.p.spade_n_up = case["latent_dim"], case["n_up"]
    opts.dis.p.ndf, opts.dis.p.n_layers, opts.dis.p.num_D = case["ndf"], case["n_layers"], case["num_D"]
    opts.dis.p.use_local_discriminator = local
    opts.dis.soft_shift, opts.dis.flip_prob = 0.0, 0.0
    opts.train.lambdas.G.p.vgg = 0
    if local:
        opts.train.lambdas.G.p.gan = 2.0
    opts.gen.p.diff_aug.update(use=diff, do_color_jittering=True, do_translation=True, do_cutout=True)
    T = Trainer(opts, device="cuda").setup(inference=False)
    T.G.painter.load_state_dict(case_state_dict(case), strict=True)
    if local:
        shapes = disc_p_shapes(3, case["ndf"], case["n_layers"], case["num_D"])
        for i, which in enumerate(("global", "local")):
            T.D["p"][which].load_state_dict({k: t(v) for k, v in fill.fill_state_dict(shapes, case["seed"] + 1 + i).items()},
                                            strict=True)
    else:
        T.D["p"].load_state_dict(gstep_d_state_dict(case), strict=True)
    T.G.set_compute_dtype(dt)
    T.D.set_compute_dtype(dt)
    T.G.painter.set_latent_shape((case["B"], 3, case["H"], case["W"]), True)
    return T


def _compare(named, gold, prefix, l2_max, cos_min, zero_tol):
    bad, checked = [], 0
    for key, p in named:
        if not p.requires_grad or key.endswith(("weight_u", "weight_v")):
            continue
        assert p.grad is not None, key
        ref = gold[prefix + key].astype(np.float64)
        got = grad_subsample(key, p.grad.detach().float().cpu(), SUB).astype(np.float64)
        base = key.rsplit(".", 1)[0]
        wkey = prefix + base + (".weight_bar" if prefix + base + ".weight_bar" in gold else ".weight")
        wscale = np.abs(gold[wkey]).max()
        if key.endswith("bias") and np.abs(ref).max() < 1e-4 * wscale:
            if np.abs(got).max() > zero_tol * wscale:
                bad.append((key, "zero-bias", np.abs(got).max() / wscale))
        else:
            l2 = np.sqrt(((got - ref) ** 2).sum() / (ref ** 2).sum())
            cos = (got * ref).sum() / np.sqrt((got ** 2).sum() * (ref ** 2).sum())
            # a one-element tensor (the last conv's bias: the sum of the real and the fake half's nearly cancelling logit
            # gradients) has no direction; its 16-bit error is bounded against the layer's weight-gradient scale instead
            scalar_ok = ref.size == 1 and abs(got[0] - ref[0]) <= zero_tol * wscale
            if not (l2 <= l2_max and cos >= cos_min) and not scalar_ok:
                bad.append((key, l2, cos))
        checked += 1
    assert not bad, (prefix, len(bad), bad[:10])
    assert checked == sum(1 for k in gold if k.startswith(prefix)), (prefix, checked)


@pytest.mark.parametrize("local", [False, True])
def test_painter_step_with_diff_aug_matches_reference(local):
    """G side then D side with diff_aug fully on, replaying the reference's recorded draws (G: the fake's, then x's; D:
    the same order): loss terms and (sub-sampled) gradients with test_gpu_train.py's bounds for these steps."""
    from climategan_amd import ops
    from climategan_amd.transforms import RecordedDraws

    case = _step_case(local)
    gold = load_golden("diffaug_step_local" if local else "diffaug_step")
    T = _trainer(case, local)
    src = RecordedDraws(_gold_draws(gold, "", int(gold["ndraws"][0])))
    T.diff_transforms.draws = src
    inp = {k: t(v).cuda() for k, v in case_inputs("gstep_p", case).items()}
    batch = {"rf": {"data": {"x": inp["x"], "m": inp["m"]}}}
    for p in T.D.parameters():
        p.requires_grad_(False)
    loss = T.get_painter_loss(batch)
    loss.backward()
    assert src.used == 14
    for key, log, tol in (("gan", "G.p.gan", 5e-3), ("featmatch", "G.p.featmatch", 1e-2)):
        ref, got = float(gold[key][0]), float(T.loss_log[log])
        assert abs(got - ref) <= tol * abs(ref), (key, got, ref)
    _compare(T.G.painter.named_parameters(), gold, "gsub.", 0.15, 0.99, 1e-2)
    # ---- D side on the reference's painted image (binary mask: the paste of it with x is itself)
    for key, p in T.D.named_parameters():
        if not key.endswith(("weight_u", "weight_v")):
            p.requires_grad_(True)
    gold_fake = t(gold["fake"]).cuda()
    if local:
        T.G.paint = lambda m, x, **kw: gold_fake
    else:
        T.G.paint_nhwc = lambda m, x: ops.nchw_to_nhwc(gold_fake, torch.float16)
    d_loss = T.get_D_loss(batch)
    d_loss.backward()
    assert src.used == 28
    if local:
        for which in ("global", "local"):
            ref, got = float(gold["d." + which][0]), float(T.loss_log["D.p." + which])
            assert abs(got - ref) <= 5e-3 * abs(ref), (which, got, ref)
        named = [("%s.%s" % (w, k), p) for w in ("global", "local") for k, p in T.D["p"][w].named_parameters()]
        _compare(named, gold, "dsub.", 0.15, 0.99, 1e-2)
    else:
        ref, got = float(gold["d.gan"][0]), float(T.loss_log["D.p.gan"])
        assert abs(got - ref) <= 2e-3 * abs(ref), (got, ref)
        _compare(T.D["p"].named_parameters(), gold, "dsub.", 8e-2, 0.997, 1e-3)


def _seeded_steps(T, batch, sd_g, sd_d, steps=2):
    from climategan_amd import ops
    T.G.load_state_dict(sd_g)
    T.D.load_state_dict(sd_d)
    ops.touch(*T.G.parameters(), *T.G.buffers(), *T.D.parameters(), *T.D.buffers())
    T.g_opt.state.clear()
    T.d_opt.state.clear()
    T.global_step = 0
    random.seed(0)
    torch.manual_seed(0)
    for _ in range(steps):
        T.train_step(batch)
    torch.cuda.synchronize()
    out = {"G." + k: v.clone() for k, v in T.G.state_dict().items()}
    out.update({"D." + k: v.clone() for k, v in T.D.state_dict().items()})
    return out, torch.cuda.get_rng_state()


@pytest.mark.parametrize("local", [False, True])
def test_seeded_steps_are_bitwise_reproducible_and_off_is_unchanged(local):
    """Two identical seeded train steps with diff_aug on give bit-identical parameters and move them away from the
    steps with it off; with ``use`` off, and with ``use`` on but every ``do_*`` off (the identity), the steps are bit for
    bit the same and draw the same random numbers."""
    from climategan_amd.transforms import DiffTransforms

    case = _step_case(local)
    T = _trainer(case, local, dt=torch.bfloat16)
    inp = {k: t(v).cuda() for k, v in case_inputs("gstep_p", case).items()}
    batch = {"rf": {"data": {"x": inp["x"], "m": inp["m"]}}}
    sd_g = {k: v.clone() for k, v in T.G.state_dict().items()}
    sd_d = {k: v.clone() for k, v in T.D.state_dict().items()}
    on1, rng_on = _seeded_steps(T, batch, sd_g, sd_d)
    on2, _ = _seeded_steps(T, batch, sd_g, sd_d)
    bad = [k for k in on1 if not torch.equal(on1[k], on2[k])]
    assert not bad, bad[:10]
    T.opts.gen.p.diff_aug.use = False
    off, rng_off = _seeded_steps(T, batch, sd_g, sd_d)
    T.opts.gen.p.diff_aug.use = True
    T.opts.gen.p.diff_aug.update(do_color_jittering=False, do_translation=False, do_cutout=False)
    T.diff_transforms = DiffTransforms(T.opts.gen.p.diff_aug)
    ident, rng_ident = _seeded_steps(T, batch, sd_g, sd_d)
    bad = [k for k in off if not torch.equal(off[k], ident[k])]
    assert not bad, bad[:10]
    assert torch.equal(rng_off, rng_ident)
    assert not torch.equal(rng_on, rng_off)                         # the augmentation draws on the device generator
    assert sum(not torch.equal(on1[k], off[k]) for k in off) > 10
