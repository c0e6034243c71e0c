"""Write tests/golden/amp_optim.npz + amp_optim_case.json by driving the optimizers the REAL reference's ``get_optimizer``
(climategan/optim.py:54-124) returns for ``optimizer: Adam`` and ``optimizer: RMSprop`` -- ``torch.optim.Adam`` /
``torch.optim.RMSprop`` -- together with ``torch.amp.GradScaler("cpu")``, the way the reference's ``train.amp`` mode does
(trainer.py:1004-1009): ``scale(loss).backward(); step(opt); update()``.  Dev container only; TEST INFRASTRUCTURE like
oracle/make_golden.py (``torch_optimizer`` is stubbed by the oracle's import recipe).

    python tests/devtools/make_golden_amp_optim.py          # from the repo root, needs the reference tree

The case (amp_optim_case.json, a ``golden_cases()``-style entry): three tensors of odd sizes in two parameter groups with
their own learning rates (the reference's per-task groups of a discriminator), weight decay on the second group; 8
iterations, counted from 1, at ``init_scale`` 65536 and ``growth_interval`` 3; +inf in the smallest tensor's gradient at
iteration 2, NaN in the last element of the largest tensor's at iteration 5.  So iterations 2 and 5 are skipped and halve
the scale, and the three clean iterations 6, 7, 8 double it.

The gradients handed to the optimizer are ``g * scale`` (what a backward of the scaled loss leaves in ``p.grad``), with
the non-finite values put in afterwards.  The file holds, per optimizer ("adam." / "rmsprop."): the initial parameters
``p<i>_init``, the unscaled gradients ``g<i>_<it>``, and after every iteration the parameters ``p<i>_after<it>``, the
moments ``m<i>_after<it>`` / ``v<i>_after<it>`` (``v`` = ``square_avg`` for RMSprop, which has no ``m``), ``steps`` [8, 3],
``scales`` [8], ``trackers`` [8] and ``found`` [8] (1 where the iteration was skipped).
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from climategan_amd import fill  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import GOLDEN_DIR, t  # noqa: E402


def case():
    return dict(kind="amp_optim", shapes=[[37, 11], [131], [5, 3, 3, 3]], groups=[[0, 1], [2]], lr=[2e-3, 5e-4],
                weight_decay=[0.0, 0.01], beta1=0.5, steps=8, init_scale=65536.0, growth_interval=3,
                inf_at=dict(step=2, tensor=1, index=7), nan_at=dict(step=5, tensor=0, index=37 * 11 - 1), seed=11)


class _Holder(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(x.clone()) for x in tensors])


def build(name, c, init):
    """The reference's get_optimizer on a two-"task" discriminator-style ModuleDict: one parameter group per task."""
    net = torch.nn.ModuleDict({"a": _Holder([init[i] for i in c["groups"][0]]), "b": _Holder([init[i] for i in c["groups"][1]])})
    conf = ref_shim.Dict(optimizer=name, beta1=c["beta1"], lr=dict(default=1e-4, a=c["lr"][0], b=c["lr"][1]),
                         lr_policy="constant")
    opt, _, names = ref_shim.ref("optim").get_optimizer(net, conf, ["a", "b"], True)
    assert names == ["disc_a", "disc_b"] and len(opt.param_groups) == 2
    for group, wd in zip(opt.param_groups, c["weight_decay"]):
        group["weight_decay"] = wd
    params = [p for g in opt.param_groups for p in g["params"]]
    return opt, params


def run(name, c):
    n = len(c["shapes"])
    init = [t(fill.uniform(tuple(s), fill.key_seed("amp_optim.p%d" % i, c["seed"]))) for i, s in enumerate(c["shapes"])]
    opt, params = build(name, c, init)
    assert type(opt) is {"Adam": torch.optim.Adam, "RMSprop": torch.optim.RMSprop}[name]
    scaler = torch.amp.GradScaler("cpu", init_scale=c["init_scale"], growth_interval=c["growth_interval"])
    out = {"p%d_init" % i: init[i].numpy().copy() for i in range(n)}
    steps, scales, trackers, found = [], [], [], []
    for it in range(1, c["steps"] + 1):
        scaler.scale(torch.zeros(()))                     # initialises the scaler's lazily built state
        scale = scaler.get_scale()
        for i, p in enumerate(params):
            g = fill.uniform(tuple(c["shapes"][i]), fill.key_seed("amp_optim.g%d_%d" % (i, it), c["seed"]), -1e-2, 1e-2)
            out["g%d_%d" % (i, it)] = g
            p.grad = t(g) * scale
        for what, value in (("inf_at", float("inf")), ("nan_at", float("nan"))):
            if c[what]["step"] == it:
                params[c[what]["tensor"]].grad.view(-1)[c[what]["index"]] = value
        before = [p.detach().clone() for p in params]
        scaler.step(opt)
        scaler.update()
        skipped = all(torch.equal(a, p.detach()) for a, p in zip(before, params))
        found.append(int(skipped))
        for i, p in enumerate(params):
            st = opt.state[p]
            out["p%d_after%d" % (i, it)] = p.detach().numpy().copy()
            if name == "Adam":
                out["m%d_after%d" % (i, it)] = st["exp_avg"].numpy().copy() if st else np.zeros_like(init[i].numpy())
            sq = "exp_avg_sq" if name == "Adam" else "square_avg"
            out["v%d_after%d" % (i, it)] = st[sq].numpy().copy() if st else np.zeros_like(init[i].numpy())
        steps.append([float(opt.state[p]["step"]) if opt.state[p] else 0.0 for p in params])
        scales.append(scaler.get_scale())
        trackers.append(scaler._get_growth_tracker())
    out["steps"] = np.array(steps, dtype=np.float64)
    out["scales"] = np.array(scales, dtype=np.float64)
    out["trackers"] = np.array(trackers, dtype=np.int64)
    out["found"] = np.array(found, dtype=np.int64)
    return out


def main():
    if not ref_shim.available():
        sys.exit("make_golden_amp_optim needs the reference tree (dev container only)")
    c = case()
    out = {}
    for name in ("Adam", "RMSprop"):
        res = run(name, c)
        assert res["found"].tolist() == [0, 1, 0, 0, 1, 0, 0, 0], res["found"]
        assert res["scales"].tolist() == [65536.0, 32768.0, 32768.0, 32768.0, 16384.0, 16384.0, 16384.0, 32768.0], res["scales"]
        out.update({name.lower() + "." + k: v for k, v in res.items()})
    path = GOLDEN_DIR / "amp_optim.npz"
    np.savez_compressed(path, **out)
    (GOLDEN_DIR / "amp_optim_case.json").write_text(json.dumps({"amp_optim": c}, indent=1) + "\n")
    print("%-20s %8d B  %d arrays" % (path.name, path.stat().st_size, len(out)))


if __name__ == "__main__":
    main()
