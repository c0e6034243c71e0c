"""Masker evaluation on the GPU (csrc/masker_eval.hip through climategan_amd.eval_metrics) against the reference's own
results (tests/golden/masker_eval.npz, made by tests/devtools/make_golden_masker_eval.py with the real
climategan.eval_metrics / climategan.data and the restated skimage 0.18.3 sobel)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from climategan_amd import eval_metrics as em

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent
Z = np.load(ROOT / "golden" / "masker_eval.npz")
META = json.loads(bytes(Z["meta"]))
CASES = sorted(k for k in META if not k.startswith("_"))
METRIC_KEYS = ("tpr", "tpt", "tnr", "tnt", "fpr", "fpt", "fnr", "fnt", "mpr", "mnr", "accuracy", "error", "precision", "f05",
               "accuracy_must_may")


def inputs(name):
    h, w = META[name]["shape"]
    label = Z["%s/label" % name].astype(np.int64)
    s = Z["%s/pred_stored" % name]
    if META[name]["soft"]:
        pred = s.astype(np.float32) / np.float32(255)
    else:
        pred = np.unpackbits(s)[: h * w].reshape(h, w).astype(bool)
    return pred, label


def same(a, b, soft):
    if soft:
        return (np.isnan(a) and np.isnan(b)) or a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b))
    return (np.isnan(a) and np.isnan(b)) or a == b


def close_ec(a, b):
    return a == b or abs(a - b) <= 1e-12 * abs(b) + 1e-15


@pytest.mark.parametrize("name", CASES)
def test_classification_metrics_match_reference(name):
    pred, label = inputs(name)
    meta = META[name]
    if "metrics_error" in meta:
        with pytest.raises(AssertionError) as e:
            em.masker_classification_metrics(pred, label)
        assert str(e.value) == meta["metrics_error"][1]
        return
    metrics, maps = em.masker_classification_metrics(pred, label)
    assert list(metrics) == list(METRIC_KEYS) and set(metrics) == set(meta["metrics"])    # the reference's key order
    for k in METRIC_KEYS:
        assert isinstance(metrics[k], np.float64), k
        assert same(float(metrics[k]), meta["metrics"][k], meta["soft"]), (k, metrics[k], meta["metrics"][k])
    assert {k: str(v.dtype) for k, v in maps.items()} == meta["maps_dtype"]
    if "%s/map_tp" % name in Z:
        for k, v in maps.items():
            assert np.array_equal(v, Z["%s/map_%s" % (name, k)]), k


@pytest.mark.parametrize("name", CASES)
def test_edge_coherence_matches_reference(name):
    pred, label = inputs(name)
    meta = META[name]
    if "edge_error" in meta:
        with pytest.raises(ValueError, match="0 sample"):
            em.edges_coherence_std_min(pred, label)
        return
    ec, pe, le = em.edges_coherence_std_min(pred, label)
    assert close_ec(float(ec), meta["edge_coherence"]), (ec, meta["edge_coherence"])
    assert type(ec).__name__ == meta["edge_coherence_type"]
    h, w = META[name]["shape"]
    assert np.array_equal(np.packbits(pe > 0), Z["%s/pred_edge_bits" % name])
    assert np.array_equal(np.packbits(le > 0), Z["%s/label_edge_bits" % name])
    if "%s/pred_sobel" % name in Z:
        assert np.array_equal(pe, Z["%s/pred_sobel" % name]) and np.array_equal(le, Z["%s/label_sobel" % name])


@pytest.mark.parametrize("name", CASES)
def test_single_metric_helpers_match_reference(name):
    pred, label = inputs(name)
    ref = META[name]["single"]
    soft = META[name]["soft"]
    fp_map, fpr = em.pred_cannot(pred, label)
    fn_map, fnr = em.missed_must(pred, label)
    mn_map, mp_map, mnr, mpr = em.may_flood(pred, label)
    tpr, tnr, precision, f1 = em.masker_metrics(pred, label)
    got = {"fpr": fpr, "fnr": fnr, "mnr": mnr, "mpr": mpr, "tpr": tpr, "tnr": tnr, "precision": precision, "f1": f1}
    for k, v in got.items():
        assert same(float(v), ref[k], soft), (k, v, ref[k])
    if "%s/map_fp" % name in Z:
        assert np.array_equal(fp_map, Z["%s/map_fp" % name]) and np.array_equal(fn_map, Z["%s/map_fn" % name])
        assert np.array_equal(mn_map, Z["%s/map_may_neg" % name]) and np.array_equal(mp_map, Z["%s/map_may_pos" % name])


def test_label_encoder_matches_reference_probe():
    probe = Z["encode/probe"]
    got = em.encode_mask_label(probe)
    assert got.dtype == np.int64 and got.shape == (1,) + probe.shape[:2]
    assert np.array_equal(got[0], Z["encode/classes"].astype(np.int64))


def test_label_encoder_argmin_on_every_colour():
    c = np.arange(256)
    img = np.stack(np.meshgrid(c, c, c, indexing="ij"), -1).reshape(4096, 4096, 3).astype(np.uint8)
    got = em.crop_resize_encode_label(img, to=None).cpu().numpy()
    a = img.astype(np.int64)
    d = np.stack([((a - np.array(v)) ** 2).sum(-1) for v in em.FLOOD_CLASSES.values()])
    assert np.array_equal(got, np.argmin(d, axis=0).astype(np.uint8))


def test_label_resize_and_crop_follow_the_image_shape():
    """eval_masker.py:190-215: the target size comes from the IMAGE's shape; skimage resize(order=0) restated:
    src = f (dst + 0.5) - 0.5 rounded half away from zero."""
    rng = np.random.default_rng(5)
    pal = np.array([[255, 0, 0], [0, 0, 255], [0, 0, 0], [200, 30, 90]], dtype=np.uint8)
    lab = pal[rng.integers(0, 4, size=(301, 517))]
    for img_hw in ((300, 520), (900, 480), (301, 517)):
        got = em.crop_resize_encode_label(lab, image_hw=img_hw, to=640).cpu().numpy()
        from climategan_amd import ops
        rows, cols, top, left = ops.resize_crop_geometry(img_hw[0], img_hw[1], 640)

        def src(n_out, n_in, off):
            s = (n_in / n_out) * (np.arange(off, off + 640) + 0.5) - 0.5
            r = np.where(s >= 0, np.floor(s + 0.5), -np.floor(-s + 0.5)).astype(np.int64)
            return np.clip(r, 0, n_in - 1)

        sub = lab[src(rows, 301, top)][:, src(cols, 517, left)].astype(np.int64)
        d = np.stack([((sub - np.array(v)) ** 2).sum(-1) for v in em.FLOOD_CLASSES.values()])
        assert np.array_equal(got, np.argmin(d, axis=0).astype(np.uint8)), img_hw


def _mixed_batch(n=64, h=96, w=80):
    """n images: fixture-like blobs with every degenerate kind mixed in (no may / no must / no cannot / blank)."""
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:h, 0:w]
    preds, labels = [], []
    for i in range(n):
        cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(8, 40)
        lab = np.where((yy - cy) ** 2 + (xx - cx) ** 2 < r * r, 1, rng.integers(0, 3, size=(h, w)) * 0)
        lab[(xx > rng.integers(0, w)) & (lab == 0)] = 2
        kind = i % 8
        if kind == 1:
            lab[lab == 2] = 0
        elif kind == 2:
            lab[lab == 1] = 0
        elif kind == 3:
            lab[lab == 0] = 2
        f = 1.0 / (1.0 + np.exp(-((r + rng.uniform(-6, 6)) ** 2 - (yy - cy - 3) ** 2 - (xx - cx) ** 2) / 60.0))
        if kind == 4:
            f[:] = 0.1
        preds.append(f.astype(np.float32))
        labels.append(lab.astype(np.int64))
    return np.stack(preds), np.stack(labels)


def _per_image(pred, label):
    """What eval_masker.py's loop computes image by image, through the mirrors (nan + exception on rejection)."""
    row = {}
    try:
        m, _ = em.masker_classification_metrics(pred, label)
        row.update({k: float(v) for k, v in m.items()})
        ok = True
    except AssertionError:
        ok = False
    try:
        row["edge_coherence"] = float(em.edges_coherence_std_min(pred, label)[0])
    except ValueError:
        ok = False
    return row if ok else None


@pytest.mark.parametrize("bin_value", [0.5, -1.0])
def test_batch_equals_per_image_mirrors(bin_value):
    preds, labels = _mixed_batch()
    r = em.masker_eval(torch.from_numpy(preds).cuda(), torch.from_numpy(labels).cuda(), bin_value=bin_value)
    assert set(em.COLUMNS) <= set(r)
    for i in range(preds.shape[0]):
        p = preds[i] > bin_value if bin_value > 0 else preds[i]
        row = _per_image(p, labels[i])
        if row is None:
            assert r["status"][i] != 0
            assert all(np.isnan(float(r[k][i])) for k in em.COLUMNS)
            continue
        assert r["status"][i] == 0
        for k in em.COLUMNS:
            assert float(r[k][i]) == row[k] or (np.isnan(row[k]) and np.isnan(float(r[k][i]))), (i, k)
    assert (r["status"] != 0).any() and (r["status"] == 0).any()


def test_batch_is_deterministic_and_batch_size_independent():
    preds, labels = _mixed_batch()
    p, lab = torch.from_numpy(preds).cuda(), torch.from_numpy(labels).cuda()
    a = em.masker_eval(p, lab, bin_value=-1.0, maps=True, edges=True)
    b = em.masker_eval(p, lab, bin_value=-1.0, maps=True, edges=True)
    for k in em.COLUMNS:
        assert np.array_equal(a[k].numpy().view(np.int64), b[k].numpy().view(np.int64)), k
    for k in ("maps", "sobel", "pred_edge", "label_edge"):
        assert torch.equal(a[k], b[k]), k
    for i in (0, 5, 33, 63):
        c = em.masker_eval(p[i:i + 1], lab[i:i + 1], bin_value=-1.0)
        for k in em.COLUMNS:
            assert np.array_equal(c[k].numpy().view(np.int64), a[k].numpy()[i:i + 1].view(np.int64)), (i, k)


def _brute_edge_coherence(pe, le):
    """Exact separable brute force in numpy: per column the nearest label-edge row, then per row the minimum over all
    columns of dx^2 + dy^2."""
    h, w = pe.shape
    ys = np.arange(h)
    g = np.full((h, w), np.inf)
    for x in range(w):
        rows = np.nonzero(le[:, x])[0]
        if rows.size:
            g[:, x] = np.abs(ys[:, None] - rows[None, :]).min(1)
    xs = np.arange(w)
    d = []
    for y in range(h):
        cols = np.nonzero(pe[y])[0]
        if cols.size:
            d2 = ((cols[:, None] - xs[None, :]) ** 2 + g[y][None, :] ** 2).min(1)
            d.append(np.sqrt(d2) / h)
    d = np.concatenate(d)
    return np.std(d), d.size


def test_noise_prediction_against_brute_force():
    """~H W / 2 prediction-edge pixels: the reference's P x L matrix would not fit in memory at 640^2."""
    rng = np.random.default_rng(3)
    pred = rng.random((256, 256)).astype(np.float32)
    label = np.zeros((256, 256), np.int64)
    yy, xx = np.mgrid[0:256, 0:256]
    label[(yy - 100) ** 2 + (xx - 140) ** 2 < 70 ** 2] = 1
    label[:, :20] = 2
    r = em.masker_eval(torch.from_numpy(pred[None]).cuda(), torch.from_numpy(label[None]).cuda(), bin_value=-1.0,
                       edges=True)
    pe, le = r["pred_edge"][0].cpu().numpy() > 0, r["label_edge"][0].cpu().numpy() > 0
    want, npx = _brute_edge_coherence(pe, le)
    assert npx == int(r["pred_edge_pixels"][0]) and npx > 256 * 256 // 3
    assert close_ec(float(r["edge_coherence"][0]), want)


def test_cli_end_to_end(tmp_path):
    """python -m climategan_amd.eval_masker on a saved run and a few generated image / label PNGs: the CSV has the
    reference's columns and equals masker_eval on the same masks."""
    import pandas as pd
    import yaml
    from PIL import Image

    from climategan_amd.apply_events import prepare_batch
    from climategan_amd.config import Opts
    from climategan_amd.trainer import Trainer

    o = Opts(yaml.safe_load((ROOT / "golden" / "ckpt_small" / "opts.yaml").read_text()))
    o.tasks = ["m"]
    run = tmp_path / "run"
    o.output_path = str(run)
    T = Trainer(o, device="cuda").setup(inference=True)
    (run / "checkpoints").mkdir(parents=True)
    torch.save({"G": T.G.state_dict()}, run / "checkpoints" / "latest_ckpt.pth")
    (run / "opts.yaml").write_text(yaml.safe_dump(json.loads(json.dumps(o))))
    rng = np.random.default_rng(8)
    (tmp_path / "imgs").mkdir()
    (tmp_path / "labels").mkdir()
    pal = np.array([[255, 0, 0], [0, 0, 255], [0, 0, 0]], dtype=np.uint8)
    imgs, labs = [], []
    for i, (h, w) in enumerate(((480, 640), (700, 660), (640, 900))):
        img = rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8)
        yy, xx = np.mgrid[0:h, 0:w]
        cls = np.where((yy - h / 2) ** 2 + (xx - w / 3) ** 2 < (h / 4) ** 2, 1, np.where(xx > 0.8 * w, 2, 0))
        Image.fromarray(img).save(tmp_path / "imgs" / ("im%d.png" % i))
        Image.fromarray(pal[cls]).save(tmp_path / "labels" / ("im%d_labeled.png" % i))
        imgs.append(img)
        labs.append(em.crop_resize_encode_label(pal[cls], image_hw=(h, w), to=640))
    cmd = [sys.executable, "-m", "climategan_amd.eval_masker", "--model", str(run), "--images_dir", str(tmp_path / "imgs"),
           "--labels_dir", str(tmp_path / "labels"), "--write_metrics", "--batch_size", "3", "--dtype", "bf16"]
    out = subprocess.run(cmd, cwd=str(ROOT.parent), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    df = pd.read_csv(run / "eval-metrics" / "eval_masker.csv", float_precision="round_trip")
    assert list(df.columns) == ["idx"] + list(em.COLUMNS) + ["filename"]
    assert list(df.filename) == ["im0.png", "im1.png", "im2.png"]
    assert (run / "eval-metrics" / "pred" / "im0_pred.png").exists() and (run / "eval-metrics" / "tp" / "im2_tp.png").exists()
    R = Trainer.resume_from_path(run, inference=True, new_exp=None, device="cuda")
    R.G.set_compute_dtype(torch.bfloat16)
    with torch.no_grad():
        m = R.G.mask(x=prepare_batch(imgs))[:, 0].float().contiguous()
    want = em.masker_eval(m, torch.stack(labs), bin_value=0.5)
    for k in em.COLUMNS:
        np.testing.assert_array_equal(df[k].to_numpy(), want[k].numpy(), err_msg=k)
