"""Write tests/golden/diffaug_*.npz by running the REAL reference's DiffAugment (climategan/transforms.py:494-626) on the
CPU (dev container only; TEST INFRASTRUCTURE, like oracle/make_golden.py whose helpers it imports).

    python tests/devtools/make_golden_diffaug.py          # from the repo root, needs the reference tree

The reference module's ``torch`` is replaced by a proxy that records the results of its ``rand`` / ``randint`` calls, so
every fixture carries the draws in call order; the tests replay them (climategan_amd.transforms.RecordedDraws) or check
that the mirror's own draw routine, seeded the same way, reproduces them.

diffaug_ops.npz      per case: the draws, the output, and the input gradient for a fixed upstream gradient (the input and
                     the upstream gradient come from the portable fill: op_inputs)
diffaug_step.npz     the Painter step of trainer.py:1256-1387 / 1073-1107 with diff_aug fully on, single multi-scale D:
                     G side (loss terms, sub-sampled Painter gradients), then the D side on the same painted image
diffaug_step_local.npz   the same with dis.p.use_local_discriminator (the local / global pair)
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from climategan_amd import fill  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import GOLDEN_DIR, _painter_opts, build_reference_module, case_inputs, grad_subsample, t  # noqa: E402

SUB = 384        # sub-sampled entries per gradient tensor (keeps each file below 1 MiB)


def op_cases():
    """name -> (N, C, H, W, color, translation ratio or None, cutout ratio or None, seed)"""
    return {
        "all_sq": (3, 3, 32, 32, True, 0.125, 0.5, 1),
        "all_odd": (3, 3, 37, 53, True, 0.125, 0.5, 2),
        "all_n1": (1, 3, 24, 40, True, 0.2, 0.3, 3),
        "color": (3, 3, 21, 30, True, None, None, 4),
        "color_n1": (1, 3, 17, 19, True, None, None, 5),
        "translation": (3, 3, 33, 21, False, 0.3, None, 6),
        "cutout": (3, 3, 31, 45, False, None, 0.5, 7),
        "cutout_big": (3, 3, 30, 41, False, None, 0.8, None),      # seed searched: boxes cross all four borders
        "cutout_zero": (3, 3, 20, 30, False, None, 0.01, 9),       # box size (0, 0)
        "cutout_zero_h": (3, 3, 20, 60, False, None, 0.02, 10),    # box size (0, 1)
    }


class RecordingTorch:
    """``torch`` for the reference's transforms module: records what rand / randint return."""

    def __init__(self):
        self.draws = []

    def __getattr__(self, k):
        return getattr(torch, k)

    def rand(self, *a, **k):
        v = torch.rand(*a, **k)
        self.draws.append(v.detach().clone())
        return v

    def randint(self, *a, **k):
        v = torch.randint(*a, **k)
        self.draws.append(v.clone())
        return v


def diff_opts(color, tr, cut):
    o = ref_shim.Dict()
    o.do_color_jittering = bool(color)
    o.do_translation = tr is not None
    o.translation_ratio = tr if tr is not None else 0.125
    o.do_cutout = cut is not None
    o.cutout_ratio = cut if cut is not None else 0.5
    return o


def op_inputs(name, n, c, h, w):
    """(x, dy) of an op case (shared with the tests)"""
    return fill.uniform((n, c, h, w), fill.key_seed(name, 1)), fill.uniform((n, c, h, w), fill.key_seed(name, 2))


def crosses_all_borders(tr_mod, seed, n, h, w, ratio):
    torch.manual_seed(seed)
    rec = RecordingTorch()
    tr_mod.torch = rec
    tr_mod.rand_cutout(torch.zeros(n, 3, h, w), ratio)
    tr_mod.torch = torch
    ch, cw = int(h * ratio + 0.5), int(w * ratio + 0.5)
    r0 = rec.draws[0].reshape(-1) - ch // 2
    c0 = rec.draws[1].reshape(-1) - cw // 2
    return bool((r0 < 0).any() and (r0 + ch > h).any() and (c0 < 0).any() and (c0 + cw > w).any())


def run_ops():
    tr_mod = ref_shim.ref("transforms")
    out = {}
    for name, (n, c, h, w, color, trr, cut, seed) in op_cases().items():
        if seed is None:
            seed = next(s for s in range(100, 10000) if crosses_all_borders(tr_mod, s, n, h, w, cut))
        x, dy = (t(a) for a in op_inputs(name, n, c, h, w))
        x.requires_grad_(True)
        rec = RecordingTorch()
        tr_mod.torch = rec
        torch.manual_seed(seed)
        y = tr_mod.DiffTransforms(diff_opts(color, trr, cut))(x)
        tr_mod.torch = torch
        y.backward(dy)
        out[name + ".meta"] = np.array([n, c, h, w, int(color), seed], dtype=np.int64)
        out[name + ".ratios"] = np.array([trr if trr is not None else -1, cut if cut is not None else -1], dtype=np.float64)
        out[name + ".y"] = y.detach().numpy()
        out[name + ".dx"] = x.grad.numpy()
        out[name + ".ndraws"] = np.array([len(rec.draws)], dtype=np.int64)
        for i, d in enumerate(rec.draws):
            out["%s.draw%d" % (name, i)] = d.numpy()
    return out


def step_case(local):
    return dict(kind="gstep_p", latent_dim=32, n_up=4, ndf=16, n_layers=3, num_D=3, H=96, W=128, B=2,
                seed=97 if local else 96, diff=dict(color=True, translation=0.125, cutout=0.5),
                **(dict(local=dict(lambda_gan=2.0)) if local else {}))


def run_step(local):
    """G side then D side, as update_G / update_D run them (the D side continues from the spectral-norm state the G side
    left, on the G side's painted image)."""
    gen = ref_shim.ref("generator")
    disc = ref_shim.ref("discriminator")
    losses = ref_shim.ref("losses")
    tutils = ref_shim.ref("tutils")
    tr_mod = ref_shim.ref("transforms")
    case = step_case(local)
    painter, _ = build_reference_module(dict(case, kind="painter"))
    painter.train()
    G = gen.OmniGenerator.__new__(gen.OmniGenerator)
    torch.nn.Module.__init__(G)
    G.opts = _painter_opts(case)
    G.painter = painter
    if local:
        opts = ref_shim.default_opts()
        opts.tasks = ["p"]
        opts.dis.p.use_local_discriminator = True
        opts.dis.p.ndf, opts.dis.p.n_layers, opts.dis.p.num_D = case["ndf"], case["n_layers"], case["num_D"]
        Dp = disc.OmniDiscriminator(opts)["p"]
        for i, which in enumerate(("global", "local")):
            shapes = {k: tuple(v.shape) for k, v in Dp[which].state_dict().items()}
            Dp[which].load_state_dict({k: t(v) for k, v in fill.fill_state_dict(shapes, case["seed"] + 1 + i).items()})
    else:
        Dp = disc.define_D(input_nc=4, ndf=case["ndf"], n_layers=case["n_layers"], norm="instance", use_sigmoid=False,
                           get_intermediate_features=True, num_D=case["num_D"])
        shapes = {k: tuple(v.shape) for k, v in Dp.state_dict().items()}
        Dp.load_state_dict({k: t(v) for k, v in fill.fill_state_dict(shapes, case["seed"] + 1).items()})
    Dp.train()
    inp = {k: t(v) for k, v in case_inputs("gstep_p", case).items()}
    x, m = inp["x"], inp["m"]
    painter.set_latent_shape(tuple(x.shape), True)
    o = ref_shim.Dict(do_color_jittering=True, do_translation=True, translation_ratio=case["diff"]["translation"],
                      do_cutout=True, cutout_ratio=case["diff"]["cutout"])
    diff = tr_mod.DiffTransforms(o)
    rec = RecordingTorch()
    tr_mod.torch = rec
    torch.manual_seed(case["seed"])
    gan, fm = losses.GANLoss(use_lsgan=False, soft_shift=0.0, flip_prob=0.0), losses.FeatMatchLoss()
    out = {}
    # ---- G side (trainer.py:1317-1385, D frozen)
    for p in Dp.parameters():
        p.requires_grad = False
    fake_flooded = G.paint(m, x)
    fake_aug = diff(fake_flooded)
    x_aug = diff(x)
    if local:
        fake_d_global = Dp["global"](fake_aug)
        fake_d_local = Dp["local"](fake_aug * m)
        real_d_global = Dp["global"](x_aug)
        l_gan = (gan(fake_d_global, True, False) + gan(fake_d_local, True, False)) * case["local"]["lambda_gan"]
        l_fm = fm(real_d_global, fake_d_global) * 10
    else:
        real_fake_d = Dp(torch.cat([torch.cat([m, x_aug], axis=1), torch.cat([m, fake_aug], axis=1)], dim=0))
        real_d, fake_d = tutils.divide_pred(real_fake_d)
        l_gan = gan(fake_d, True, False)
        l_fm = fm(real_d, fake_d) * 10
    loss = l_gan + l_fm
    loss.backward()
    out.update({"loss": loss.detach().numpy().reshape(1), "gan": l_gan.detach().numpy().reshape(1),
                "featmatch": l_fm.detach().numpy().reshape(1), "fake": fake_flooded.detach().numpy()})
    for key, p in painter.named_parameters():
        if p.requires_grad:
            out["gsub." + key] = grad_subsample(key, p.grad, SUB)
    # ---- D side (trainer.py:1073-1107) on the same painted image
    for key, p in Dp.named_parameters():
        if not key.endswith(("weight_u", "weight_v")):
            p.requires_grad = True
    with torch.no_grad():
        fake = diff(fake_flooded.detach())
        xd = diff(x)
    gan_d = losses.GANLoss(use_lsgan=False, soft_shift=0.0, flip_prob=0.0)
    if local:
        g_loss = gan_d(Dp["global"](fake), False, True) + gan_d(Dp["global"](xd), True, True)
        l_loss = gan_d(Dp["local"](fake * m), False, True) + gan_d(Dp["local"](xd * m), True, True)
        (g_loss + l_loss).backward()
        out["d.global"], out["d.local"] = g_loss.detach().numpy().reshape(1), l_loss.detach().numpy().reshape(1)
        named = [("%s.%s" % (w, k), p) for w in ("global", "local") for k, p in Dp[w].named_parameters()]
    else:
        real_d, fake_d = tutils.divide_pred(Dp(torch.cat([torch.cat([m, xd], axis=1), torch.cat([m, fake], axis=1)], dim=0)))
        d_loss = gan_d(fake_d, False, True) + gan_d(real_d, True, True)
        d_loss.backward()
        out["d.gan"] = d_loss.detach().numpy().reshape(1)
        named = list(Dp.named_parameters())
    for key, p in named:
        if p.grad is not None and not key.endswith(("weight_u", "weight_v")):
            out["dsub." + key] = grad_subsample(key, p.grad, SUB)
    tr_mod.torch = torch
    out["ndraws"] = np.array([len(rec.draws)], dtype=np.int64)
    for i, d in enumerate(rec.draws):
        out["draw%d" % i] = d.numpy()
    return out


def main():
    if not ref_shim.available():
        sys.exit("make_golden_diffaug needs the reference tree (dev container only)")
    torch.set_num_threads(8)
    for name, fn in (("diffaug_ops", run_ops), ("diffaug_step", lambda: run_step(False)),
                     ("diffaug_step_local", lambda: run_step(True))):
        out = fn()
        path = GOLDEN_DIR / (name + ".npz")
        np.savez_compressed(path, **out)
        print("%-20s %8d B  %d arrays" % (name, path.stat().st_size, len(out)))


if __name__ == "__main__":
    main()
