"""Mirror of the decode half of the reference's ``climategan/data.py`` (:21-148, :212-252, :344-399): what happens between
the file and the transforms.  File reading stays PIL / numpy on the host; everything that touches pixels is the gather of
csrc/data_tf.hip with a raw source kind (``transforms.RawSource``), so ``tensor_loader`` here is the identity-plan launch
of the kernel ``compile_transforms`` uses for a whole batch -- hand the ``RawSource`` itself to the batch form and the
full-resolution decode never happens.

The reference reads images with ``imageio.imread``; here ``numpy.array(PIL.Image.open(path))`` takes its place (the same
array for the 8-bit RGB / RGBA / grey and the 16-bit grey PNGs the datasets hold), ``numpy.load`` reads ``.npy`` and
``torch.load`` passes ``.pt`` segmentation maps through.

``classes_dict`` and ``kitti_mapping`` restate the reference's tables as data; tests/golden/data_decode.npz records the
reference's own and the host test compares.

Out of scope: ``OmniListDataset`` / ``get_loader`` and the Logger's display helpers (``decode_segmap_merged_labels``, ...).
"""
from pathlib import Path

import numpy as np
import torch

from . import ops
from .transforms import RawSource

classes_dict = {
    "s": {0: [0, 0, 255, 255], 1: [55, 55, 55, 255], 2: [0, 255, 255, 255], 3: [255, 212, 0, 255], 4: [0, 255, 0, 255],
          5: [255, 97, 0, 255], 6: [255, 0, 0, 255], 7: [60, 180, 60, 255], 8: [255, 0, 255, 255], 9: [0, 0, 0, 255],
          10: [255, 255, 255, 255]},
    "r": {0: [0, 0, 255, 255], 1: [55, 55, 55, 255], 2: [0, 255, 255, 255], 3: [255, 212, 0, 255], 4: [0, 255, 0, 255],
          5: [255, 97, 0, 255], 6: [255, 0, 0, 255], 7: [60, 180, 60, 255], 8: [220, 20, 60, 255], 9: [8, 19, 49, 255],
          10: [0, 80, 100, 255]},
    "kitti": {0: [210, 0, 200], 1: [90, 200, 255], 2: [0, 199, 0], 3: [90, 240, 0], 4: [140, 140, 140], 5: [100, 60, 100],
              6: [250, 100, 255], 7: [255, 255, 0], 8: [200, 200, 0], 9: [255, 130, 0], 10: [80, 80, 80], 11: [160, 60, 60],
              12: [255, 127, 80], 13: [0, 139, 139], 14: [0, 0, 0]},
    "flood": {0: [255, 0, 0], 1: [0, 0, 255], 2: [0, 0, 0]},
}

kitti_mapping = {0: 5, 1: 9, 2: 7, 3: 4, 4: 2, 5: 1, 6: 3, 7: 3, 8: 3, 9: 3, 10: 10, 11: 6, 12: 6, 13: 6, 14: 10}

IMG_EXTENSIONS = (".jpg", ".jpeg", ".png", ".ppm", ".bmp", ".tif", ".tiff")


def _device(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def read_array(path):
    """The array as the decoder leaves it: ``np.load`` for ``.npy``, else ``np.array(PIL.Image.open(path))`` (the call that
    replaces the reference's ``imageio.imread``)"""
    path = Path(path)
    if path.suffix == ".npy":
        return np.load(path)
    if path.suffix.lower() in IMG_EXTENSIONS:
        from PIL import Image
        return np.array(Image.open(path))
    raise ValueError("Unknown data type {}".format(path))


def _on_device(source, device=None):
    """(device array, whether the caller gave numpy) of a path, a numpy array or a tensor"""
    if isinstance(source, (str, Path)):
        source = read_array(source)
    if isinstance(source, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(source)).to(_device(device)), True
    return source, False


def _like(tensor, as_numpy):
    return tensor.cpu().numpy() if as_numpy else tensor


def exact_palette(classes, merge_map=None, default_value=14):
    """The by-value table of the exact lookup: colour -> label (data.py:104-107), or with ``merge_map`` colour -> merged
    label (:123-126 folded in: a label outside the map, the default included, becomes ``default_value``)"""
    def merged(label):
        return label if merge_map is None else merge_map.get(label, default_value)
    return ops.data_palette(list(classes.values()), [merged(c) for c in classes], merged(default_value))


_NEAREST = {}


def nearest_palette(domain):
    """The table of ``encode_segmap`` for ``domain``, in the dict's order: ``find_closest_class``'s strict ``<`` keeps the
    first class at the smallest distance (data.py:221-228)"""
    if domain not in _NEAREST:
        classes = classes_dict[domain]
        _NEAREST[domain] = ops.data_palette(list(classes.values()), list(classes))
    return _NEAREST[domain]


def encode_exact_segmap(seg, classes_dict, default_value=14, device=None):
    """reference data.py:91-107: H x W x 3 uint8 -> H x W float64 labels, ``default_value`` where no colour matches.  numpy
    in, numpy out; a device tensor in, a device tensor out."""
    t, as_numpy = _on_device(seg, device)
    src = RawSource(t, "kitti_s", palette=exact_palette(classes_dict, None, default_value))
    return _like(src.to_tensor()[0, 0], as_numpy)


def merge_labels(labels, mapping, default_value=14):
    """reference data.py:110-126, on the host (numpy in, numpy out): a table lookup over a label map.  The loaders never
    call it on its own: ``process_kitti_seg`` folds the map into the colour table of the one launch."""
    out = np.ones_like(labels) * default_value
    for source, target in mapping.items():
        out[labels == source] = target
    return out


def process_kitti_seg(path, kitti_classes, merge_map, default=14, device=None):
    """reference data.py:129-148: a path or an H x W x 3 uint8 array -> the 1 x 1 x H x W float64 segmap on the device"""
    return kitti_seg_source(path, kitti_classes, merge_map, default, device).to_tensor()


def kitti_seg_source(source, kitti_classes=None, merge_map=None, default=14, device=None):
    t, _ = _on_device(source, device)
    palette = exact_palette(kitti_classes or classes_dict["kitti"], merge_map or kitti_mapping, default)
    return RawSource(t, "kitti_s", palette=palette)


def encode_segmap(arr, domain, device=None):
    """reference data.py:231-252: H x W x 4 uint8 RGBA -> 1 x H x W float64 class ids (numpy in, numpy out; tensor in, tensor
    out).  The kernel writes the fp32 ids of ``transform_segmap_image_to_tensor`` (:274-283); the float64 is a cast."""
    t, as_numpy = _on_device(arr, device)
    ids = RawSource(t, "palette_s", palette=nearest_palette(domain)).to_tensor()[0]
    return _like(ids.double(), as_numpy)


def raw_source(source, task, domain, opts, device=None):
    """The ``RawSource`` of what ``tensor_loader`` would decode: hand it to ``compile_transforms`` instead of the tensor"""
    t, _ = _on_device(source, device)
    if task == "s":
        if domain == "kitti":
            return kitti_seg_source(t)
        return RawSource(t, "palette_s", palette=nearest_palette(domain))
    if task == "d":
        normalize = "d" in opts.train.pseudo.tasks                                      # data.py:365-370
        log = bool(opts.gen.d.classify.enable)
        if domain == "r":
            return RawSource(t if t.dtype == torch.float32 else t.float(), "f32_d")     # arr.astype(np.float32), data.py:364
        return RawSource(t, "unity_d" if domain == "s" else "kitti_d", log=log, normalize=normalize)
    if task == "x":
        return RawSource(t, "x")
    if task == "m":
        return RawSource(t, "mask")
    raise ValueError("tensor_loader: no raw form of task %r" % (task,))


def tensor_loader(source, task, domain, opts, device=None):
    """reference data.py:344-399: ``source`` (a path, or the array as the image decoder returns it, numpy or device tensor)
    -> the reference's [1, C, H, W] tensor on the device.  ``.pt`` segmentation maps pass through ``torch.load``."""
    if task == "s" and domain != "kitti" and isinstance(source, (str, Path)) and Path(source).suffix == ".pt":
        return torch.load(source)
    return raw_source(source, task, domain, opts, device).to_tensor()
