"""Host-side mirror of the reference's ``climategan/eval_metrics.py`` validation metrics used by
``Trainer.eval_images`` (trainer.py:1706-1790): ``accuracy`` (eval_metrics.py:67-76) and ``mIOU`` (eval_metrics.py:79-130).

The reference moves predictions to the CPU and loops over classes with ``.item()`` synchronisations; here one HIP kernel
(``cgan_seg_counts``) produces the per-class counts (predicted / labelled / both) in one pass over the device tensors
and the ratios are formed from 3 x C integers.  Integer work: results are exactly the reference's for the same logits.
"""

import numpy as np
import torch

from . import _lib, ops


def _counts(pred, label):
    """pred: ``ops.NHWC`` logits or an [N, C, H, W] device tensor; label: [N, H, W] or [N, 1, H, W]."""
    if isinstance(pred, ops.NHWC):
        n, hw, c, layout, dtype, p = pred.n, pred.h * pred.w, pred.c, 0, pred.dtype_id, pred.t
        if pred.cs != ops.cs8(c):
            raise RuntimeError("metrics: NHWC logits must be stored with round_up(c, 8) channels")
    else:
        if pred.dim() != 4:
            raise ValueError("metrics: [N, C, H, W] logits expected, got %s" % (tuple(pred.shape),))
        p = pred.contiguous().float()
        n, c, layout, dtype = p.shape[0], p.shape[1], 1, 0
        hw = p.shape[2] * p.shape[3]
    ops._need_cuda(p, label)
    if label.dim() == 4:
        assert label.shape[1] == 1                                    # eval_metrics.py:70-72
        label = label[:, 0]
    if label.numel() != n * hw:
        raise ValueError("metrics: %d labels for %d predictions" % (label.numel(), n * hw))
    lab = label.contiguous().float()
    counts = torch.zeros((3, c), dtype=torch.int64, device=p.device)
    lib = _lib.load()
    _lib.check(lib.cgan_seg_counts(ops._ptr(p), layout, dtype, n, hw, c, ops._ptr(lab), ops._ptr(counts), ops._stream()),
               "cgan_seg_counts")
    return counts.cpu().numpy(), n * hw, lab


def accuracy(pred_im, gt_im):
    """eval_metrics.py:67-76: ``(argmax_c(pred) == gt).sum() / gt.size``.

    Reproduced as the reference computes it, quirks included: the label array is taken BEFORE its channel axis is
    squeezed, so (i) with [N, 1, H, W] labels and N > 1 the comparison broadcasts across samples -- refused here, pass
    [N, H, W] labels or one sample at a time as ``Trainer.eval_images`` does; (ii) a 1-channel prediction (the binarised
    mask of trainer.py:1763-1768) is arg-maxed to all zeros, so its "accuracy" is the fraction of zero labels."""
    n = pred_im.n if isinstance(pred_im, ops.NHWC) else pred_im.shape[0]
    c = pred_im.c if isinstance(pred_im, ops.NHWC) else pred_im.shape[1]
    if gt_im.dim() == 4 and n > 1:
        raise NotImplementedError("accuracy: [N, 1, H, W] labels with N > 1 broadcast across samples in the reference "
                                  "(eval_metrics.py:68-76); pass [N, H, W] labels or single samples")
    if c == 1:
        if isinstance(pred_im, ops.NHWC):
            raise NotImplementedError("accuracy: 1-channel NHWC predictions are not used by the reference's callers")
        pred_im = torch.cat([pred_im.float() * 0 + 1, pred_im.float() * 0], dim=1)     # argmax == 0 everywhere
    counts, total, _ = _counts(pred_im, gt_im)
    return float(counts[2].sum()) / total


def mIOU(pred, label, average="macro"):
    """eval_metrics.py:79-130 (pred: logits; label: integer class map).  With 2 classes only ``label.max()`` is scored;
    classes absent from both prediction and label are skipped; nan when nothing is left."""
    counts, _, lab = _counts(pred, label)
    num_classes = counts.shape[1]
    interesting = list(range(num_classes)) if num_classes > 2 else [int(lab.max().item())]
    weights, ious = [], []
    for k in interesting:
        n_pred = int(counts[0][k]) if 0 <= k < num_classes else 0
        n_tgt = int(counts[1][k]) if 0 <= k < num_classes else 0
        if n_tgt > 0 or n_pred > 0:
            inter = int(counts[2][k])
            weights.append(n_pred)
            ious.append(float(inter) / float(n_pred + n_tgt - inter))
    if not ious:
        return float("nan")
    if average == "weighted":
        return np.sum(np.multiply(weights, ious) / np.sum(weights))
    return np.mean(ious)


# ------------------------------------------------------------------------------------------------------------------------
# Masker evaluation on a labelled test set (reference eval_masker.py, eval_metrics.py:133-542).
#
# The per-pixel work -- the six masked sums of masker_classification_metrics, the label counts, the Sobel edges of
# edges_coherence_std_min and the exact distance of every prediction-edge pixel to the "must" label edge -- is one
# ``cgan_masker_eval`` call per batch (csrc/masker_eval.hip, six launches).  The ratios are finished here with numpy
# float64 scalars in the reference's operation order, so 0 / 0 is nan as in numpy and, for binary predictions (exact
# integer sums), every column but edge_coherence is bit-identical to the reference's.
# ------------------------------------------------------------------------------------------------------------------------

MEVAL_U8, MEVAL_F64 = 3, 4                 # cgan_masker_eval's extra prediction dtypes (include/climategan_hip.h)
COLUMNS = ("tpr", "tpt", "tnr", "tnt", "fpr", "fpt", "fnr", "fnt", "mnr", "mpr", "accuracy", "error", "precision", "f05",
           "accuracy_must_may", "edge_coherence")                # eval_masker.py:512-531
STATUS_ASSERT = 1            # masker_classification_metrics' np.isclose assertions fail (a class is absent: nan rates)
STATUS_NO_LABEL_EDGE = 2     # prediction edges but no "must" label edge: euclidean_distances raises ValueError
FLOOD_CLASSES = {0: [255, 0, 0], 1: [0, 0, 255], 2: [0, 0, 0]}     # data.py:65-69 classes_dict["flood"]
_MAP_NAMES = ("tp", "tn", "fp", "fn", "may_pos", "may_neg")


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _as_tensor(a):
    if isinstance(a, torch.Tensor):
        return a
    return torch.from_numpy(np.ascontiguousarray(a))


def _pred_kind(t):
    """(C-ABI dtype id, numpy-equivalent dtype of the comparison ``pred > th``)."""
    d = t.dtype
    if d == torch.float32:
        return _lib.CGAN_F32, np.float32
    if d == torch.float16:
        return _lib.CGAN_F16, np.float16
    if d == torch.bfloat16:
        return _lib.CGAN_BF16, "bf16"
    if d == torch.float64:
        return MEVAL_F64, np.float64
    if d in (torch.bool, torch.uint8):
        return MEVAL_U8, np.float16
    raise TypeError("masker_eval: prediction dtype %s is not supported (fp32, fp16, bf16, fp64, bool, uint8)" % d)


def _round_threshold(th, kind):
    """The threshold as ``pred > th`` sees it under numpy 1.x value-based casting (the reference's numpy): a Python float
    against a float32 / float16 array is compared in that type, against a bool / uint8 array in float16 (0.5 is exact in
    all of them); a bf16 tensor compares in bf16 as torch does."""
    if kind == "bf16":
        return float(torch.tensor(float(th), dtype=torch.bfloat16).float())
    return float(kind(th))


def _label_u8(label, labels_dict=None):
    """Class ids -> uint8 0 cannot / 1 must / 2 may / 3 none on the device (any integer label array or tensor)."""
    t = _as_tensor(label)
    if not t.is_cuda:
        t = t.to(_device())
    if labels_dict is None and t.dtype == torch.uint8:
        return t.contiguous()
    ids = labels_dict or {"cannot": 0, "must": 1, "may": 2}
    out = torch.full(t.shape, 3, dtype=torch.uint8, device=t.device)
    for code, key in enumerate(("cannot", "must", "may")):
        if key in ids and ids[key] is not None:
            out[t == ids[key]] = code
    return out


def _launch(pred, label, binarize, bin_value, edge_th, maps=False, sobel=False):
    """One ``cgan_masker_eval`` over a [N, H, W] batch -> (res int64 [N, 16] on the device, pred_edge, label_edge, maps,
    sobel)."""
    p = _as_tensor(pred)
    if not p.is_cuda:
        p = p.to(_device())
    if p.dim() == 2:
        p = p[None]
    if p.dim() == 4 and p.shape[1] == 1:
        p = p[:, 0]
    if p.dim() != 3:
        raise ValueError("masker_eval: [N, H, W] predictions expected, got %s" % (tuple(p.shape),))
    lab = label if (isinstance(label, torch.Tensor) and label.dtype == torch.uint8 and label.is_cuda) else _label_u8(label)
    if lab.dim() == 2:
        lab = lab[None]
    if tuple(lab.shape) != tuple(p.shape):
        raise ValueError("masker_eval: labels %s do not match predictions %s" % (tuple(lab.shape), tuple(p.shape)))
    dtype_id, kind = _pred_kind(p)
    if p.dtype == torch.bool:
        p = p.view(torch.uint8)
    p, lab = p.contiguous(), lab.contiguous()
    ops._need_cuda(p, lab)
    n, h, w = p.shape
    dev = p.device
    pe = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    le = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    res = torch.empty((n, 16), dtype=torch.int64, device=dev)
    mp = torch.empty((6, n, h, w), dtype=torch.float64, device=dev) if maps else None
    sb = torch.empty((2, n, h, w), dtype=torch.float64, device=dev) if sobel else None
    lib = _lib.load()
    nb = lib.cgan_masker_eval_workspace_bytes(n, h, w)
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    _lib.check(lib.cgan_masker_eval(ops._ptr(p), dtype_id, ops._ptr(lab), n, h, w, int(bool(binarize)),
                                    _round_threshold(bin_value, kind), _round_threshold(edge_th, kind), ops._ptr(pe),
                                    ops._ptr(le), ops._ptr(mp), ops._ptr(sb), ops._ptr(res), ops._ptr(ws), nb,
                                    ops._stream()), "cgan_masker_eval")
    return res, pe, le, mp, sb


def _finish(res, h, w):
    """Host finish of ``res`` (numpy int64 [N, 16]) -> list of per-image dicts of numpy float64 scalars, in the
    reference's operation order (eval_metrics.py:204-238), plus the raw edge statistics."""
    flt = np.ascontiguousarray(res[:, 8:]).view(np.float64)
    total = np.prod(np.array([h, w], dtype=np.int64))            # np.prod(label.shape)
    out = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(res.shape[0]):
            n_cannot, n_must, n_may = (np.int64(v) for v in res[i, 0:3])
            tp, tn, fp, fn, mp, mn = (np.float64(v) for v in flt[i, 0:6])
            tpr = tp / n_must
            tpt = tp / total
            tnr = tn / n_cannot
            tnt = tn / total
            fpr = fp / n_cannot
            fpt = fp / total
            fnr = fn / n_must
            fnt = fn / total
            mnr = mn / n_may
            mpr = mp / n_may
            accuracy = tpt + tnt
            error = fpt + fnt
            precision = tp / (tp + fp + 1e-9)
            beta = 0.5
            f05 = ((1 + beta ** 2) * precision * tpr) / (beta ** 2 * precision + tpr + 1e-9)
            accuracy_must_may = (tp + mn) / (n_must + n_may)
            out.append({
                "tpr": tpr, "tpt": tpt, "tnr": tnr, "tnt": tnt, "fpr": fpr, "fpt": fpt, "fnr": fnr, "fnt": fnt,
                "mpr": mpr, "mnr": mnr, "accuracy": accuracy, "error": error, "precision": precision, "f05": f05,
                "accuracy_must_may": accuracy_must_may,
                "_sums": (tp, tn, fp, fn, mp, mn), "_counts": (n_cannot, n_must, n_may),
                "_edges": (int(res[i, 6]), int(res[i, 7]), np.float64(flt[i, 7])),
            })
    return out


def _classification_assert(m):
    """eval_metrics.py:214-217: the reference's assertions, messages included (None when they pass)."""
    if not np.isclose(m["tpr"], 1.0 - m["fnr"]):
        return "TPR: {:.4f}, FNR: {:.4f}".format(m["tpr"], m["fnr"])
    if not np.isclose(m["tnr"], 1.0 - m["fpr"]):
        return "TNR: {:.4f}, FPR: {:.4f}".format(m["tnr"], m["fpr"])
    if not np.isclose(m["mpr"], 1.0 - m["mnr"]):
        return "MPR: {:.4f}, MNR: {:.4f}".format(m["mpr"], m["mnr"])
    return None


def _status(m):
    pe, le, _ = m["_edges"]
    return (STATUS_ASSERT if _classification_assert(m) else 0) | (STATUS_NO_LABEL_EDGE if pe > 0 and le == 0 else 0)


def _edge_value(m):
    pe, le, std = m["_edges"]
    if pe == 0:
        return 1.0                                    # eval_metrics.py:533-535
    if le == 0:
        return float("nan")
    return std


def _maps_dtype(pred):
    """numpy's result dtypes of ``pred * int_array`` and ``(1.0 - pred) * int_array`` for this prediction."""
    d = pred.dtype
    integer = (d in (torch.bool, torch.uint8)) if isinstance(pred, torch.Tensor) else (d == np.bool_ or d == np.uint8)
    return (np.int64, np.float64) if integer else (np.float64, np.float64)


def _host_maps(mp, pred):
    """fp64 [6, 1, H, W] device maps -> the reference's maps_dict (tp / fp / may_pos int64 for bool predictions)."""
    pos_t, neg_t = _maps_dtype(pred)
    a = mp[:, 0].cpu().numpy()
    out = {}
    for k, name in enumerate(_MAP_NAMES):
        out[name] = a[k].astype(neg_t if name in ("tn", "fn", "may_neg") else pos_t)
    return out


def masker_eval(pred, label, bin_value=0.5, maps=False, edges=False):
    """Batched masker evaluation (eval_masker.py:505-560 for N images at once).

    pred: [N, H, W] (or [N, 1, H, W]) masks -- fp32 / fp16 / bf16 / fp64 / bool / uint8, numpy or tensor; label: [N, H, W]
    integer class ids (0 cannot, 1 must, 2 may).  ``bin_value > 0`` binarises the prediction as eval_masker does
    (``pred > bin_value``, eval_masker.py:507-508) before every metric; otherwise the sums are soft and the edge map uses
    edges_coherence_std_min's default ``pred > 0.5``.

    Returns a dict of per-image float64 CPU tensors, one per column of the reference's CSV (``COLUMNS``), plus
    ``status`` (int32: STATUS_ASSERT | STATUS_NO_LABEL_EDGE, 0 = the reference accepts the image) and the edge pixel
    counts.  An image the reference rejects gets nan in every column.  ``maps=True`` adds ``maps`` (fp64 [6, N, H, W]
    device tensor: tp tn fp fn may_pos may_neg); ``edges=True`` adds ``pred_edge`` / ``label_edge`` (uint8 edge masks)
    and ``sobel`` (fp64 [2, N, H, W] magnitude maps).  Six kernel launches and one device-to-host copy per call."""
    binarize = bin_value > 0
    res, pe, le, mp, sb = _launch(pred, label, binarize, bin_value if binarize else 0.5, 0.5, maps=maps, sobel=edges)
    h, w = pe.shape[1], pe.shape[2]
    per = _finish(res.cpu().numpy(), h, w)
    cols = {k: np.empty(len(per), dtype=np.float64) for k in COLUMNS}
    status = np.zeros(len(per), dtype=np.int32)
    for i, m in enumerate(per):
        status[i] = _status(m)
        for k in COLUMNS[:-1]:
            cols[k][i] = m[k]
        cols["edge_coherence"][i] = _edge_value(m)
        if status[i]:
            for k in COLUMNS:
                cols[k][i] = np.nan
    out = {k: torch.from_numpy(v) for k, v in cols.items()}
    out["status"] = torch.from_numpy(status)
    out["pred_edge_pixels"] = torch.tensor([m["_edges"][0] for m in per], dtype=torch.int64)
    out["label_edge_pixels"] = torch.tensor([m["_edges"][1] for m in per], dtype=torch.int64)
    if maps:
        out["maps"] = mp
    if edges:
        out["pred_edge"], out["label_edge"], out["sobel"] = pe, le, sb
    return out


def masker_classification_metrics(pred, label, labels_dict={"cannot": 0, "must": 1, "may": 2}):
    """eval_metrics.py:133-238 for one [H, W] prediction: (metrics_dict, maps_dict), same keys, dtypes and
    AssertionErrors as the reference."""
    res, _, _, mp, _ = _launch(pred, _label_u8(label, labels_dict), False, 0.5, 0.5, maps=True)
    h, w = mp.shape[2], mp.shape[3]
    m = _finish(res.cpu().numpy(), h, w)[0]
    msg = _classification_assert(m)
    if msg is not None:
        raise AssertionError(msg)
    metrics = {k: m[k] for k in ("tpr", "tpt", "tnr", "tnt", "fpr", "fpt", "fnr", "fnt", "mpr", "mnr", "accuracy", "error",
                                 "precision", "f05", "accuracy_must_may")}
    return metrics, _host_maps(mp, pred)


def _single(pred, label, labels_dict):
    res, _, _, mp, _ = _launch(pred, _label_u8(label, labels_dict), False, 0.5, 0.5, maps=True)
    return _finish(res.cpu().numpy(), mp.shape[2], mp.shape[3])[0], _host_maps(mp, pred)


def pred_cannot(pred, label, label_cannot=0):
    """eval_metrics.py:241-266: (fp_map, fpr)."""
    m, maps = _single(pred, label, {"cannot": label_cannot})
    return maps["fp"], m["fpr"]


def missed_must(pred, label, label_must=1):
    """eval_metrics.py:269-294: (fn_map, fnr)."""
    m, maps = _single(pred, label, {"must": label_must})
    return maps["fn"], m["fnr"]


def may_flood(pred, label, label_may=2):
    """eval_metrics.py:297-331: (may_neg_map, may_pos_map, mnr, mpr)."""
    m, maps = _single(pred, label, {"may": label_may})
    return maps["may_neg"], maps["may_pos"], m["mnr"], m["mpr"]


def masker_metrics(pred, label, label_cannot=0, label_must=1):
    """eval_metrics.py:334-373: (tpr, tnr, precision, f1) -- precision and f1 without the 1e-9 of the classification
    metrics."""
    res, _, _, _, _ = _launch(pred, _label_u8(label, {"cannot": label_cannot, "must": label_must}), False, 0.5, 0.5)
    p = _as_tensor(pred)
    m = _finish(res.cpu().numpy(), p.shape[-2], p.shape[-1])[0]
    tp, tn, fp, fn, _, _ = m["_sums"]
    with np.errstate(divide="ignore", invalid="ignore"):
        precision = tp / (tp + fp)
        f1 = 2 * (precision * m["tpr"]) / (precision + m["tpr"])
    return m["tpr"], m["tnr"], precision, f1


def get_confusion_matrix(tpr, tnr, fpr, fnr, mpr, mnr):
    """eval_metrics.py:376-459 (host-only numpy): means and population standard deviations over images,
    [i, j] = [pred, true]: | tnr fnr mnr | fpr tpr mpr | 0 0 0 |."""
    tpr_m, tpr_s = np.mean(tpr), np.std(tpr)
    tnr_m, tnr_s = np.mean(tnr), np.std(tnr)
    fpr_m, fpr_s = np.mean(fpr), np.std(fpr)
    fnr_m, fnr_s = np.mean(fnr), np.std(fnr)
    mpr_m, mpr_s = np.mean(mpr), np.std(mpr)
    mnr_m, mnr_s = np.mean(mnr), np.std(mnr)
    assert np.isclose(tpr_m, 1.0 - fnr_m), "TPR: {:.4f}, FNR: {:.4f}".format(tpr_m, fnr_m)
    assert np.isclose(tnr_m, 1.0 - fpr_m), "TNR: {:.4f}, FPR: {:.4f}".format(tnr_m, fpr_m)
    assert np.isclose(mpr_m, 1.0 - mnr_m), "MPR: {:.4f}, MNR: {:.4f}".format(mpr_m, mnr_m)
    confusion_matrix = np.zeros((3, 3))
    confusion_matrix[0, 0] = tnr_m
    confusion_matrix[0, 1] = fnr_m
    confusion_matrix[0, 2] = mnr_m
    confusion_matrix[1, 0] = fpr_m
    confusion_matrix[1, 1] = tpr_m
    confusion_matrix[1, 2] = mpr_m
    confusion_matrix[2, 2] = 0.0
    confusion_matrix_std = np.zeros((3, 3))
    confusion_matrix_std[0, 0] = tnr_s
    confusion_matrix_std[0, 1] = fnr_s
    confusion_matrix_std[0, 2] = mnr_s
    confusion_matrix_std[1, 0] = fpr_s
    confusion_matrix_std[1, 1] = tpr_s
    confusion_matrix_std[1, 2] = mpr_s
    confusion_matrix_std[2, 2] = 0.0
    return confusion_matrix, confusion_matrix_std


def edges_coherence_std_min(pred, label, label_must=1, bin_th=0.5):
    """eval_metrics.py:484-542 for one [H, W] prediction: (edge_coherence, pred_sobel, label_sobel).  The exact distance
    transform replaces the reference's P x L distance matrix; a blank prediction gives 1.0, prediction edges without a
    "must" label edge raise the ValueError the reference's euclidean_distances raises on an empty set."""
    lab = _label_u8(label, {"must": label_must})
    res, _, _, _, sb = _launch(pred, lab, False, 0.5, bin_th, sobel=True)
    r = res.cpu().numpy()
    pe, le = int(r[0, 6]), int(r[0, 7])
    std = np.ascontiguousarray(r[0, 8:]).view(np.float64)[7]
    ps, ls = sb[0, 0].cpu().numpy(), sb[1, 0].cpu().numpy()
    if pe == 0:
        return 1.0, ps, ls
    if le == 0:
        raise ValueError("Found array with 0 sample(s) (shape=(0, 2)) while a minimum of 1 is required by "
                         "check_pairwise_arrays.")
    return np.float64(std), ps, ls


def encode_mask_label(arr, domain="flood"):
    """data.py:255-271 for the "flood" domain: an RGB [H, W, 3] uint8 label image -> int64 [1, H, W] class ids (the
    nearest of ``FLOOD_CLASSES``, first index on ties), computed on the device."""
    if domain != "flood":
        raise NotImplementedError("encode_mask_label: only the 'flood' domain is evaluated here")
    t = _as_tensor(arr)
    h, w = t.shape[0], t.shape[1]
    return crop_resize_encode_label(t, (h, w), to=None).cpu().numpy().astype(np.int64)[None]


def crop_resize_encode_label(label, image_hw=None, to=640):
    """eval_masker.py:168-229 (label branch) + encode_mask_label: RGB uint8 [H, W, 3] label photo -> uint8 [to, to] class
    ids on the device.  The resize target comes from ``image_hw`` (the IMAGE's height and width, a reference quirk:
    ``l_h, l_w = img.shape[:2]``; default: the label's own); nearest neighbour as skimage 0.18.3
    ``resize(order=0, preserve_range=True)`` (restated from its source, not pinned against an installed copy), then the
    centre crop.  ``to=None``: no resize and no crop (plain ``encode_mask_label``)."""
    t = _as_tensor(label)
    if t.dtype != torch.uint8:
        raise ValueError("crop_resize_encode_label: uint8 label image expected, got %s" % t.dtype)
    if t.dim() != 3 or t.shape[2] != 3:
        raise ValueError("crop_resize_encode_label: an RGB [H, W, 3] label image is expected, got %s (convert RGBA / grey "
                         "labels first; the reference's encode_mask_label fails on them)" % (tuple(t.shape),))
    if not t.is_cuda:
        t = t.to(_device())
    t = t.contiguous()
    h, w = t.shape[0], t.shape[1]
    if to is None:
        rows, cols, top, left, oh, ow = h, w, 0, 0, h, w
    else:
        ih, iw = image_hw if image_hw is not None else (h, w)
        rows, cols, top, left = ops.resize_crop_geometry(int(ih), int(iw), to)
        oh = ow = to
    out = torch.empty((oh, ow), dtype=torch.uint8, device=t.device)
    lib = _lib.load()
    _lib.check(lib.cgan_mask_label_encode(ops._ptr(t), 1, h, w, 3, rows, cols, top, left, oh, ow, ops._ptr(out),
                                          ops._stream()), "cgan_mask_label_encode")
    return out
