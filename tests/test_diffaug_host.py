"""CPU tests of the DiffAugment mirror (climategan_amd/transforms.py; reference climategan/transforms.py:494-626): its draw
routine consumes the random stream exactly as the reference does (fixture tests/golden/diffaug_ops.npz, written by
tests/devtools/make_golden_diffaug.py from the reference's own recorded torch.rand / randint results), the Trainer no
longer refuses gen.p.diff_aug, and the new C-ABI symbols are declared, exported and bound."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import load_golden

ROOT = Path(__file__).resolve().parent.parent


def _opts(color, tr, cut):
    from climategan_amd.config import default_opts
    o = default_opts().gen.p.diff_aug
    o.do_color_jittering = bool(color)
    o.do_translation = tr >= 0
    o.translation_ratio = tr if tr >= 0 else 0.125
    o.do_cutout = cut >= 0
    o.cutout_ratio = cut if cut >= 0 else 0.5
    return o


class _Recording:
    def __init__(self):
        from climategan_amd.transforms import TorchDraws
        self.inner, self.draws = TorchDraws(), []

    def rand(self, *a):
        self.draws.append(self.inner.rand(*a))
        return self.draws[-1]

    def randint(self, *a):
        self.draws.append(self.inner.randint(*a))
        return self.draws[-1]


def _op_case_names(gold):
    return sorted(k[:-5] for k in gold if k.endswith(".meta"))


def test_draws_reproduce_the_reference_stream_bit_for_bit():
    from climategan_amd.transforms import DiffTransforms

    gold = load_golden("diffaug_ops")
    names = _op_case_names(gold)
    assert len(names) >= 10
    for name in names:
        n, c, h, w, color, seed = (int(v) for v in gold[name + ".meta"])
        tr, cut = (float(v) for v in gold[name + ".ratios"])
        rec = _Recording()
        torch.manual_seed(seed)
        p = DiffTransforms(_opts(color, tr, cut), draws=rec).draw(n, h, w, torch.device("cpu"))
        assert p is not None
        assert len(rec.draws) == int(gold[name + ".ndraws"][0]), name
        for i, d in enumerate(rec.draws):
            ref = gold["%s.draw%d" % (name, i)]
            got = d.numpy()
            assert got.shape == ref.shape and got.dtype == ref.dtype, (name, i, got.shape, got.dtype, ref.shape, ref.dtype)
            assert np.array_equal(got, ref), (name, i)


def test_params_carry_the_draws_and_the_box_size():
    from climategan_amd import ops
    from climategan_amd.transforms import RecordedDraws, draw_params

    draws = [torch.tensor([[[[0.25]]], [[[0.5]]]]), torch.tensor([[[[0.75]]], [[[0.0]]]]), torch.tensor([[[[1.0]]], [[[0.125]]]]),
             torch.tensor([[[3]], [[-2]]]), torch.tensor([[[0]], [[1]]]), torch.tensor([[[5]], [[0]]]), torch.tensor([[[9]], [[11]]])]
    src = RecordedDraws(draws)
    p = draw_params(2, 20, 30, torch.device("cpu"), color=(True, True, True), translation_ratio=0.125, cutout_ratio=0.5,
                    draws=src)
    assert src.used == 7
    assert p.flags == ops.DA_BRIGHTNESS | ops.DA_CONTRAST | ops.DA_SATURATION | ops.DA_TRANSLATION | ops.DA_CUTOUT
    assert p.cut_hw == (10, 15)
    assert p.color.dtype == torch.float32 and p.color.tolist() == [[0.25, 0.75, 1.0], [0.5, 0.0, 0.125]]
    assert p.geo.dtype == torch.int64 and p.geo.tolist() == [[3, 0, 5, 9], [-2, 1, 0, 11]]
    with pytest.raises(RuntimeError):
        RecordedDraws(draws[:1]).randint(0, 3, 2, "cpu")          # a draw of the wrong shape is refused


def test_all_ops_off_is_the_identity_and_draws_nothing():
    from climategan_amd.transforms import DiffTransforms

    dt = DiffTransforms(_opts(False, -1, -1))
    assert not dt.active
    x = torch.rand(2, 3, 8, 8)
    state = torch.get_rng_state()
    assert dt(x) is x
    assert dt.draw(2, 8, 8, torch.device("cpu")) is None
    assert torch.equal(state, torch.get_rng_state())


def test_non_diffaugment_branches_raise():
    from climategan_amd import transforms as T

    x = torch.rand(1, 3, 4, 4)
    for fn in (T.rand_brightness, T.rand_contrast, T.rand_saturation):
        with pytest.raises(NotImplementedError):
            fn(x)


class _Painted(Exception):
    pass


class _StubG:
    """stands in for G: the Painter call is where a configuration the Trainer accepts starts computing"""

    class painter:
        compute_dtype = torch.bfloat16

    def paint_nhwc(self, m, x):
        raise _Painted()

    def paint(self, m, x):
        raise _Painted()


@pytest.mark.parametrize("local", [False, True])
def test_trainer_accepts_diff_aug(local):
    from climategan_amd.config import default_opts
    from climategan_amd.trainer import Trainer
    from climategan_amd.transforms import DiffTransforms

    opts = default_opts()
    opts.tasks = ["p"]
    opts.dis.p.use_local_discriminator = local
    opts.gen.p.diff_aug.update(use=True, do_color_jittering=True, do_translation=True, do_cutout=True)
    T = Trainer(opts, device="cpu")
    T.diff_transforms = DiffTransforms(opts.gen.p.diff_aug)          # what setup() builds for this configuration
    T.G = _StubG()
    T.losses = {"G": {"p": {"vgg": None}}}
    T.loss_log = {}
    batch = {"rf": {"data": {"x": torch.zeros(1, 3, 8, 8), "m": torch.zeros(1, 1, 8, 8)}}}
    with pytest.raises(_Painted):
        T.get_painter_loss(batch)
    with pytest.raises(_Painted):
        T.get_D_loss(batch)
    assert T._diff_aug() is T.diff_transforms
    opts.gen.p.diff_aug.update(do_color_jittering=False, do_translation=False, do_cutout=False)
    T.diff_transforms = DiffTransforms(opts.gen.p.diff_aug)
    assert T._diff_aug() is None                                        # every do_* off: the identity


def test_new_symbols_are_declared_exported_and_bound():
    from climategan_amd import _lib

    names = ["cgan_diffaug_fwd", "cgan_diffaug_bwd", "cgan_painter_heads_diffaug_fwd", "cgan_painter_heads_diffaug_bwd"]
    header = (ROOT / "include" / "climategan_hip.h").read_text()
    declared = set(re.findall(r"\b(cgan_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for name in names:
        assert name in declared, name
        assert name in _lib._SIGNATURES, name
        assert getattr(lib, name) is not None
    assert re.search(r"#define CGAN_DIFFAUG_PARTS 256\b", header)
    from climategan_amd import ops
    assert ops.DIFFAUG_PARTS == 256
    for bit, name in ((ops.DA_BRIGHTNESS, "BRIGHTNESS"), (ops.DA_CONTRAST, "CONTRAST"), (ops.DA_SATURATION, "SATURATION"),
                      (ops.DA_TRANSLATION, "TRANSLATION"), (ops.DA_CUTOUT, "CUTOUT")):
        assert re.search(r"#define CGAN_DA_%s %d\b" % (name, bit), header), name
