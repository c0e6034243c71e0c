"""Masker evaluation, host side (no GPU): the committed fixture, ``get_confusion_matrix``, the CLI's argument handling,
pairing and ``--load_metrics`` skip, ``Trainer.resume_from_path`` on a run saved by ``Trainer.save``, and the exact
integer distance recurrence of csrc/masker_eval.hip restated in numpy against a brute force."""
import importlib.util
import json
import shutil
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

from climategan_amd import eval_masker, eval_metrics

ROOT = Path(__file__).resolve().parent
GOLDEN = ROOT / "golden" / "masker_eval.npz"


def _generator():
    spec = importlib.util.spec_from_file_location("make_golden_masker_eval", ROOT / "devtools" / "make_golden_masker_eval.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixture_is_current():
    z = np.load(GOLDEN)
    meta = json.loads(bytes(z["meta"]))
    gen = _generator()
    assert GOLDEN.stat().st_size < 1 << 20
    assert set(gen.CASES) == {k for k in meta if not k.startswith("_")}
    for name, (h, w, soft, _, _) in gen.CASES.items():
        assert meta[name]["shape"] == [h, w] and meta[name]["soft"] == soft
        assert z["%s/label" % name].shape == (h, w) and z["%s/label" % name].dtype == np.uint8
        stored = z["%s/pred_stored" % name]
        assert stored.dtype == np.uint8 and stored.size == (h * w if soft else (h * w + 7) // 8)
        assert ("metrics" in meta[name]) != ("metrics_error" in meta[name])
        assert ("edge_coherence" in meta[name]) != ("edge_error" in meta[name])
    assert z["encode/classes"].shape == z["encode/probe"].shape[:2]


def test_confusion_matrix_matches_reference():
    z = np.load(GOLDEN)
    cm, cs = eval_metrics.get_confusion_matrix(*(z["confusion/in_%s" % k] for k in ("tpr", "tnr", "fpr", "fnr", "mpr", "mnr")))
    assert np.array_equal(cm, z["confusion/mean"]) and np.array_equal(cs, z["confusion/std"])
    bad = json.loads(bytes(z["meta"]))["_confusion_bad"]
    with pytest.raises(AssertionError, match="^%s$" % bad[1].replace(".", r"\.")):
        eval_metrics.get_confusion_matrix(*(z["confusion/in_%s" % k] for k in ("tpr", "tnr", "fpr", "fnr")),
                                          z["confusion/in_mnr"], z["confusion/in_mnr"] * 0)


@pytest.mark.parametrize("arg", ["--tags", "-t", "--plot", "--no_paint", "--prepare_torch", "--output_csv=x.csv"])
def test_cli_refuses_reference_only_arguments(arg):
    with pytest.raises(SystemExit, match="not supported"):
        eval_masker.parse_args(["--model", "m", "--images_dir", "i", "--labels_dir", "l", arg])


def test_cli_argument_checks():
    a = eval_masker.parse_args(["--model", "m", "--images_dir", "i", "--labels_dir", "l"])
    assert (a.bin_value, a.max_files, a.batch_size, a.dtype, a.write_metrics, a.load_metrics) == (0.5, -1, 16, "split24",
                                                                                                  False, False)
    for bad in (["--image_size", "512"], ["--dtype", "fp32"], ["--batch_size", "0"]):
        with pytest.raises(SystemExit):
            eval_masker.parse_args(["--model", "m", "--images_dir", "i", "--labels_dir", "l"] + bad)
    with pytest.raises(SystemExit):
        eval_masker.parse_args(["--images_dir", "i", "--labels_dir", "l"])


def _touch(d, names):
    d.mkdir(parents=True, exist_ok=True)
    for n in names:
        (d / n).write_bytes(b"")


def test_cli_pairing_rule(tmp_path):
    _touch(tmp_path / "i", ["b.jpg", "a.png", "c.JPG", "notes.txt", "a_b.png"])
    _touch(tmp_path / "l", ["c_labeled.png", "a_labeled.png", "b_labeled.png", "a_b_labeled.png", "x.yaml"])
    imgs, labs = eval_masker.pair_paths(tmp_path / "i", tmp_path / "l")
    assert [p.name for p in imgs] == ["a.png", "a_b.png", "b.jpg", "c.JPG"]
    # eval_masker.py:427-430: sorted with "_labeled." removed ("a." < "a_b."; the plain names would sort a_b_ first)
    assert [p.name for p in labs] == ["a_labeled.png", "a_b_labeled.png", "b_labeled.png", "c_labeled.png"]
    imgs, labs = eval_masker.pair_paths(tmp_path / "i", tmp_path / "l", max_files=2)
    assert len(imgs) == len(labs) == 2


def test_cli_load_metrics_skips_evaluated_models(tmp_path, capsys):
    from PIL import Image

    (tmp_path / "i").mkdir()
    (tmp_path / "l").mkdir()
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "i" / "a.png")
    Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(tmp_path / "l" / "a_labeled.png")
    run = tmp_path / "run"
    (run / "eval-metrics" / "pred").mkdir(parents=True)
    (run / "eval-metrics" / "eval_masker.csv").write_text("idx\n")
    frames = eval_masker.main(["--model", str(run), "--images_dir", str(tmp_path / "i"), "--labels_dir",
                               str(tmp_path / "l"), "--load_metrics"])
    assert frames == []
    assert "Skipping model because pre-computed metrics exist" in capsys.readouterr().out


def test_cli_refuses_rgba(tmp_path):
    from PIL import Image

    Image.fromarray(np.zeros((8, 8, 4), np.uint8)).save(tmp_path / "rgba.png")
    Image.fromarray(np.zeros((8, 8), np.uint8)).save(tmp_path / "grey.png")
    for n in ("rgba.png", "grey.png"):
        with pytest.raises(ValueError, match="not an 8-bit RGB image"):
            eval_masker.read_rgb(tmp_path / n, "label")


def test_resume_from_path(tmp_path):
    """trainer.py:337-394: the latest ``opts (i).yaml`` + overrides, ``train.resume``, setup, checkpoint loaded."""
    from climategan_amd.config import Opts
    from climategan_amd.trainer import Trainer

    fix = ROOT / "golden" / "ckpt_small"
    o = Opts(yaml.safe_load((fix / "opts.yaml").read_text()))
    o.output_path = str(tmp_path)
    o.train.lambdas.G.p.vgg = 0
    T = Trainer(o, device="cpu").setup(inference=False)
    with torch.no_grad():
        for i, p in enumerate(T.G.parameters()):
            p.add_(0.001 * (i + 1))
    T.epoch, T.global_step = 3, 7
    T.save()
    plain = json.loads(json.dumps(o))
    (tmp_path / "opts.yaml").write_text(yaml.safe_dump(plain))
    plain["train"]["save_n_epochs"] = 99
    (tmp_path / "opts (1).yaml").write_text(yaml.safe_dump(plain))
    R = Trainer.resume_from_path(tmp_path, overrides={"train": {"min_save_epoch": 5}}, inference=True, new_exp=None,
                                 device="cpu")
    assert R.opts.train.save_n_epochs == 99 and R.opts.train.min_save_epoch == 5 and R.opts.train.resume is True
    assert R.opts.events.fire.kernel_size == 281
    ref = T.G.state_dict()
    assert all(torch.equal(R.G.state_dict()[k], v) for k, v in ref.items())
    with pytest.warns(UserWarning):       # torch's scheduler-before-optimizer note, as in test_checkpoint
        R2 = Trainer.resume_from_path(tmp_path, device="cpu")
    assert (R2.epoch, R2.global_step) == (3, 8)          # the step is rounded up to an even number
    shutil.rmtree(tmp_path / "checkpoints")
    with pytest.raises(AssertionError):
        Trainer.resume_from_path(tmp_path, device="cpu")


def column_row_distance(le, pe):
    """csrc/masker_eval.hip passes 3-4 in numpy: g = vertical distance to the nearest label edge of the column, then per
    prediction-edge pixel min_x' (x - x')^2 + g(x', y)^2 with the kernel's outward search and early stop."""
    h, w = le.shape
    none = 0x3FFFFFFF
    g = np.full((h, w), none, dtype=np.int64)
    for x in range(w):
        last = -1
        for y in range(h):
            if le[y, x]:
                last = y
            g[y, x] = none if last < 0 else y - last
        nxt = -1
        for y in range(h - 1, -1, -1):
            if le[y, x]:
                nxt = y
            if nxt >= 0:
                g[y, x] = min(g[y, x], nxt - y)
    out = np.full((h, w), -1, dtype=np.int64)
    for y, x in zip(*np.nonzero(pe)):
        best = None
        for d in range(w):
            if best is not None and d * d >= best:
                break
            for xx in ((x - d,) if d == 0 else (x - d, x + d)):
                if 0 <= xx < w and g[y, xx] != none:
                    v = d * d + int(g[y, xx]) ** 2
                    best = v if best is None or v < best else best
        out[y, x] = best
    return out


@pytest.mark.parametrize("seed,h,w,p", [(0, 17, 23, 0.05), (1, 9, 31, 0.3), (2, 31, 7, 0.01), (3, 1, 19, 0.2),
                                        (4, 20, 20, 0.002)])
def test_distance_recurrence_is_exact(seed, h, w, p):
    rng = np.random.default_rng(seed)
    le = rng.random((h, w)) < p
    if not le.any():
        le[rng.integers(h), rng.integers(w)] = True
    pe = rng.random((h, w)) < 0.3
    got = column_row_distance(le, pe)
    ly, lx = np.nonzero(le)
    for y, x in zip(*np.nonzero(pe)):
        assert got[y, x] == int(((ly - y) ** 2 + (lx - x) ** 2).min())
