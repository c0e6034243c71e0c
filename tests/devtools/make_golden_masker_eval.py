"""Write tests/golden/masker_eval.npz by running the REAL reference's masker metrics (climategan/eval_metrics.py:133-542)
and label encoder (climategan/data.py:255-271) on the CPU (dev container only; TEST INFRASTRUCTURE, like
make_golden_diffaug.py).

    python tests/devtools/make_golden_masker_eval.py      # from the repo root, needs the reference tree

scikit-image is not installed: ``skimage.filters.sobel`` is the 0.18.3 source restated below (scipy.ndimage.convolve,
reflect mode, outer row / column zeroed, sqrt(h^2 + v^2) / sqrt(2)); sklearn's ``euclidean_distances`` is the real one.

Inputs come from a seeded recipe (``case_inputs``) and are stored compressed: uint8 labels, bool predictions as packed
bits, soft predictions as uint8 q with pred = float32(q) / float32(255).  Stored per case: the inputs, the 15 metrics or
the reference's exception, the metric maps and Sobel maps of the small cases, the packed-bit edge masks, the edge
coherence or its exception, and the single-metric helpers' values.
"""
import json
import sys
import types
from pathlib import Path

import numpy as np
from scipy import ndimage

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402

OUT = ROOT / "tests" / "golden" / "masker_eval.npz"
HSOBEL = np.array([[1, 2, 1], [0, 0, 0], [-1, -2, -1]]) / 4.0


def _mask_filter_result(result):
    result[0, :] = 0
    result[-1, :] = 0
    result[:, 0] = 0
    result[:, -1] = 0
    return result


def sobel_0183(image):
    """skimage 0.18.3 filters.sobel(image, mask=None) on a float64 image."""
    image = np.asarray(image, dtype=np.float64)
    h = _mask_filter_result(ndimage.convolve(image, HSOBEL))
    v = _mask_filter_result(ndimage.convolve(image, HSOBEL.T))
    out = np.sqrt(h ** 2 + v ** 2)
    out /= np.sqrt(2)
    return out


def blobs(rng, h, w, k, scale):
    """A smooth random field: k Gaussian bumps of random sign, centre and width."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w))
    for _ in range(k):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        s = rng.uniform(0.05, 0.25) * scale
        f += rng.choice([-1.0, 1.0]) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return f


def blob_label(rng, h, w):
    f, g = blobs(rng, h, w, 6, max(h, w)), blobs(rng, h, w, 6, max(h, w))
    lab = np.where(f > 0.1, 1, 0)
    lab[(np.abs(g) > 0.4) & (lab == 0)] = 2
    return lab.astype(np.uint8)


# name -> (h, w, soft, seed, variant)
CASES = {
    "blob640_bool": (640, 640, False, 1, None),
    "blob640_soft": (640, 640, True, 2, None),
    "odd_bool": (37, 53, False, 3, None),
    "odd_soft": (37, 53, True, 4, None),
    "row_1xN": (1, 57, False, 5, "row"),
    "col_Nx1": (41, 1, True, 6, "row"),
    "no_may": (48, 40, False, 7, "no_may"),
    "no_must": (40, 48, False, 8, "no_must"),
    "no_cannot": (44, 44, True, 9, "no_cannot"),
    "blank_pred": (50, 60, False, 10, "blank"),
    "border_pred": (45, 39, False, 11, "border"),
    "must_only_edge": (30, 30, False, 12, "must_blank_label"),
}


def case_inputs(name):
    """-> (pred, label, stored pred form): bool pred, or float32 q / 255 from uint8 q."""
    h, w, soft, seed, variant = CASES[name]
    rng = np.random.default_rng(seed)
    if variant == "row":
        label = rng.integers(0, 3, size=(h, w)).astype(np.uint8)
    else:
        label = blob_label(rng, h, w)
    if variant == "no_may":
        label[label == 2] = 0
    if variant == "no_must":
        label[label == 1] = 2
    if variant == "no_cannot":
        label[label == 0] = 2
    if variant == "must_blank_label":
        label[:] = 2
        label[h // 3: 2 * h // 3, :] = 0
    f = blobs(rng, h, w, 5, max(h, w)) + 0.3 * (label == 1)
    q = np.clip(np.round(255.0 / (1.0 + np.exp(-6.0 * f))), 0, 255).astype(np.uint8)
    if variant == "blank":
        q[:] = 0
    if variant == "border":
        q[:] = 0
        q[0, :] = 255
        q[:, -1] = 255
        q[h // 2: h // 2 + 5, w // 3: w // 3 + 7] = 255
    if soft:
        return q.astype(np.float32) / np.float32(255), label, q
    pred = q > 127
    return pred, label, np.packbits(pred)


def colour_probe():
    """Every colour of {0, 1, 127, 128, 254, 255}^3 (the ties of the flood palette among them) + 4096 random ones."""
    v = np.array([0, 1, 127, 128, 254, 255], dtype=np.uint8)
    grid = np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3)
    rnd = np.random.default_rng(99).integers(0, 256, size=(4096, 3)).astype(np.uint8)
    return np.concatenate([grid, rnd]).reshape(77, 56, 3)


def main():
    em = ref_shim.ref("eval_metrics")
    em.filters = types.SimpleNamespace(sobel=sobel_0183)
    data = ref_shim.ref("data")
    out, meta = {}, {}
    for name in CASES:
        pred, label, stored = case_inputs(name)
        out["%s/label" % name] = label
        out["%s/pred_stored" % name] = stored
        m = {"shape": list(label.shape), "soft": bool(CASES[name][2])}
        label = label.astype(np.int64)                   # what encode_mask_label's np.argmin hands eval_masker
        try:
            metrics, maps = em.masker_classification_metrics(pred, label)
            m["metrics"] = {k: float(v) for k, v in metrics.items()}
            m["maps_dtype"] = {k: str(v.dtype) for k, v in maps.items()}
            if pred.size <= 64 * 64:
                for k, v in maps.items():
                    out["%s/map_%s" % (name, k)] = v
        except AssertionError as e:
            m["metrics_error"] = ["AssertionError", str(e)]
        try:
            ec, pe, le = em.edges_coherence_std_min(pred, label)
            m["edge_coherence"] = float(ec)
            m["edge_coherence_type"] = type(ec).__name__
            out["%s/pred_edge_bits" % name] = np.packbits(pe > 0)
            out["%s/label_edge_bits" % name] = np.packbits(le > 0)
            if pred.size <= 64 * 64:
                out["%s/pred_sobel" % name] = pe
                out["%s/label_sobel" % name] = le
        except ValueError as e:
            m["edge_error"] = ["ValueError", str(e)]
        fp_map, fpr = em.pred_cannot(pred, label)
        fn_map, fnr = em.missed_must(pred, label)
        mn_map, mp_map, mnr, mpr = em.may_flood(pred, label)
        with np.errstate(all="ignore"):
            tpr, tnr, precision, f1 = em.masker_metrics(pred, label)
        m["single"] = {"fpr": float(fpr), "fnr": float(fnr), "mnr": float(mnr), "mpr": float(mpr), "tpr": float(tpr),
                       "tnr": float(tnr), "precision": float(precision), "f1": float(f1)}
        meta[name] = m
    # confusion matrices over the accepted cases, and one that asserts
    ok = [meta[n]["metrics"] for n in meta if "metrics" in meta[n]]
    cols = {k: np.array([d[k] for d in ok]) for k in ("tpr", "tnr", "fpr", "fnr", "mpr", "mnr")}
    cm, cs = em.get_confusion_matrix(cols["tpr"], cols["tnr"], cols["fpr"], cols["fnr"], cols["mpr"], cols["mnr"])
    out["confusion/mean"], out["confusion/std"] = cm, cs
    for k, v in cols.items():
        out["confusion/in_%s" % k] = v
    try:
        em.get_confusion_matrix(cols["tpr"], cols["tnr"], cols["fpr"], cols["fnr"], cols["mnr"], cols["mnr"] * 0)
        meta["_confusion_bad"] = None
    except AssertionError as e:
        meta["_confusion_bad"] = ["AssertionError", str(e)]
    # label encoder on a colour probe (ties included)
    probe = colour_probe()
    out["encode/probe"] = probe
    out["encode/classes"] = np.squeeze(data.encode_mask_label(probe, "flood")).astype(np.uint8)
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, OUT.stat().st_size))


if __name__ == "__main__":
    main()
