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

**The loaders** (``data.py:402-539``): ``OmniListDataset`` reads the file lists; ``get_loader`` returns an
``OmniLoader`` -- an iterable of collated batches, not a ``torch.utils.data.DataLoader``: its workers are THREADS that read
and decode files into numpy arrays, one batch ahead of the consumer; the arrays of a task travel through one pinned
buffer and one copy on a side stream, and the whole batch is then the one launch per task of ``compile_transforms``.
With ``data.loaders.decode: device`` the threads only read and probe the PNG and JPEG files, and the batch's
files are decoded by the device decoders (``png.py``, ``jpeg.py``) in one call per codec.

Out of scope: the Logger's display helpers (``decode_segmap_merged_labels``, ...).
"""
import collections
import ctypes as C
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np
import torch

from . import _lib, jpeg, ops, parallel, png
from .transforms import Compose, RawSource, compile_transforms, get_transforms, set_draws
from .utils import env_to_path

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


# ----------------------------------------------------------------------------------------------------------------------
# The datasets and loaders (reference data.py:402-539)
# ----------------------------------------------------------------------------------------------------------------------
MAX_WORKERS = 16        # reader threads of one loader, whatever the machine's CPU count


def read_host(path, task, domain):
    """The host half of ``raw_source``: ``(array, known)`` with the contiguous numpy array the device half wraps (the
    fourth channel of ``x`` and ``m`` dropped, the real domain's depth as fp32: data.py:364, 382-383) and what a pass over
    the array tells while it is in the cache -- ``minmax`` of ``x`` and of the real depth, the mask's ``threshold`` --
    so that no launch has to find them.  A ``.pt`` segmentation map is returned as the tensor ``torch.load`` gives."""
    path = Path(path)
    if task == "s" and domain != "kitti" and path.suffix == ".pt":
        return torch.load(path), {}
    arr = read_array(path)
    known = {}
    if task in ("x", "m") and arr.ndim == 3 and arr.shape[-1] == 4:
        arr = arr[:, :, :3]
    if task == "d" and domain == "r":
        arr = arr.astype(np.float32, copy=False)
    arr = np.ascontiguousarray(arr)
    if task == "x" or (task == "d" and domain == "r"):
        known["minmax"] = (arr.min(), arr.max())
    elif task == "m":
        known["threshold"] = bool(arr.max() > 127)
    return arr, known


DECODE_MODES = ("host", "device")

# A file a reader thread leaves to the device decoders (``decode="device"``): ``codec`` "png" or "jpeg", the
# descriptor its ``probe`` filled, ``stream`` the bytes the decoder reads (a PNG file's zlib stream, a JPEG file as it is) and,
# for a row-framed PNG candidate, its ``c_uint32`` table of row offsets; ``path``: the file, should the host have to read it
FileRecord = collections.namedtuple("FileRecord", "codec desc stream table path")


def raw_kind(task, domain):
    """The ``ops.RAW_KINDS`` name ``raw_source`` wraps a decoded file of ``task`` in; None where the host converts the array
    first (the real domain's depth) or the task has no raw form"""
    if task in ("x", "m"):
        return "x" if task == "x" else "mask"
    if task == "s":
        return "kitti_s" if domain == "kitti" else "palette_s"
    if task == "d" and domain != "r":
        return "unity_d" if domain == "s" else "kitti_d"
    return None


def device_takes(task, domain, channels, bit_depth):
    """Whether the array a device decoder leaves of such a file -- [H, W] for one channel, [H, W, C] otherwise, uint8 or
    uint16 -- is one the task's raw kind accepts (``ops.RAW_KINDS``): x: 8 bits, 3 or 4 channels; m: 8 bits; s: 8-bit RGBA
    (kitti: RGB); d: 8 bits with 3 or 4 channels in the simulated domain, 16-bit grey in kitti."""
    kind = raw_kind(task, domain)
    if kind is None:
        return False
    _, _, dtype, dims, chans = ops.RAW_KINDS[kind]
    nd = 2 if channels == 1 else 3
    return dtype == {8: "uint8", 16: "uint16"}.get(bit_depth) and nd in dims and (chans is None or nd == 2 or channels in chans)


def read_file(path, task, domain):
    """``read_host`` for a loader that decodes on the device: a ``FileRecord`` for a PNG or JPEG file a device decoder takes
    (``png.probe`` / ``jpeg.probe``, host only) and whose array the task accepts (``device_takes``); for every other file
    exactly what ``read_host`` returns, so that whatever it raises comes from the same place."""
    path = Path(path)
    suffix = path.suffix.lower()
    if suffix == ".png":
        data = path.read_bytes()
        d, _ = png.probe(data)
        if d is not None and device_takes(task, domain, d.channels, d.bit_depth):
            return FileRecord("png", d, png.stream_of(data, d), png.row_table(data, d) if d.rows else None, path)
    elif suffix in (".jpg", ".jpeg") and task == "x":
        data = path.read_bytes()
        d, _ = jpeg.probe(data)
        if d is not None and device_takes(task, domain, d.ncomp, 8):
            return FileRecord("jpeg", d, data, None, path)
    return read_host(path, task, domain)


class OmniListDataset:
    """reference data.py:402-504: the samples of one ``opts.data.files[mode][domain]`` list (``.json`` or ``.yaml``; a
    name without ``/`` is looked up in ``opts.data.files.base``), cut to ``opts.data.max_samples``, each reduced to the
    tasks of ``opts.tasks`` (+ ``x``, + ``m`` with the Painter).  ``dataset[i]`` is the reference's item through the
    per-sample path (``tensor_loader`` + ``Compose(get_transforms(...))``); ``read_raw(i)`` gives the sample as the
    ``RawSource``s the batch transform reads."""

    def __init__(self, mode, domain, opts, transform=None, device=None):
        import yaml

        self.opts, self.domain, self.mode, self.device = opts, domain, mode, device
        self.tasks = set(opts.tasks)
        self.tasks.add("x")
        if "p" in self.tasks:
            self.tasks.add("m")
        file_list_path = list_path(opts, mode, domain)
        with open(file_list_path, "r") as f:
            if file_list_path.suffix == ".json":
                self.samples_paths = json.load(f)
            elif file_list_path.suffix in {".yaml", ".yml"}:
                self.samples_paths = yaml.safe_load(f)
            else:
                raise ValueError("Unknown file list type in {}".format(file_list_path))
        max_samples = opts.data.get("max_samples")
        if max_samples and max_samples != -1:
            assert isinstance(max_samples, int)
            self.samples_paths = self.samples_paths[:max_samples]
        self.filter_samples()
        if opts.data.get("check_samples"):
            print(f"Checking samples ({mode}, {domain})")
            self.check_samples()
        self.file_list_path = str(file_list_path)
        self.transform = transform if transform is not None else Compose(get_transforms(opts, mode, domain))

    def filter_samples(self):
        """data.py:437-444: only the files of the model's tasks"""
        self.samples_paths = [{k: v for k, v in s.items() if k in self.tasks} for s in self.samples_paths]

    def check_samples(self):
        """data.py:497-503: every listed file exists"""
        for s in self.samples_paths:
            for k, v in s.items():
                assert Path(v).exists(), f"{k} {v} does not exist"

    def __len__(self):
        return len(self.samples_paths)

    def __getitem__(self, i):
        paths = self.samples_paths[i]
        data = {task: tensor_loader(env_to_path(path), task, self.domain, self.opts, self.device)
                for task, path in paths.items()}
        return {"data": self.transform(data), "paths": paths, "domain": self.domain if self.domain != "kitti" else "s",
                "mode": self.mode}

    def read_host(self, i):
        """{task: (array, known)} of sample ``i``: the part of ``read_raw`` that runs in a reader thread"""
        return {task: read_host(env_to_path(path), task, self.domain) for task, path in self.samples_paths[i].items()}

    def read_file(self, i):
        """``read_host`` of a loader with ``decode="device"``: {task: FileRecord, or (array, known) as ``read_host`` gives}"""
        return {task: read_file(env_to_path(path), task, self.domain) for task, path in self.samples_paths[i].items()}

    def wrap(self, task, array, known=None):
        """The ``RawSource`` of a device array of this dataset's ``task`` (a ``.pt`` map stays the tensor it is)"""
        if array.is_floating_point() and array.dim() == 4:
            return array
        return raw_source(array, task, self.domain, self.opts).set_known(**(known or {}))

    def read_raw(self, i, device=None):
        """{task: RawSource} of sample ``i`` on the device: the file through ``read_array`` on the host, the array as it is
        to the device; the decode happens in the gather that reads it"""
        dev = _device(device if device is not None else self.device)
        return {task: self.wrap(task, (v if torch.is_tensor(v) else torch.from_numpy(v)).to(dev), known)
                for task, (v, known) in self.read_host(i).items()}


class _Slot:
    """One batch in flight: per task a pinned staging buffer and its device copy, the event recorded behind the upload
    and the event recorded behind the gather that read the device copy"""

    ALIGN = 256         # every sample starts on a boundary the 16-byte loads of the min / max kernels accept

    def __init__(self):
        self.pinned, self.dev = {}, {}
        self.uploaded = self.consumed = None
        self.decoded = None             # decode="device": the decoder calls' outputs that the staged arrays are views of

    def buffers(self, task, nbytes, device):
        if task not in self.pinned or self.pinned[task].numel() < nbytes:
            size = max(nbytes + nbytes // 4, 1 << 16)
            self.pinned[task] = torch.empty(size, dtype=torch.uint8).pin_memory()
            self.dev[task] = torch.empty(size, dtype=torch.uint8, device=device)
        return self.pinned[task], self.dev[task]


class OmniLoader:
    """What ``get_loader`` returns: an iterable of the reference's collated batches ``{"data": {task: [N, C, h, w] device
    tensor}, "paths": {task: [path] * N}, "domain": [domain] * N, "mode": [mode] * N}`` with ``len()``, ``.dataset`` and
    ``.batch_size``; ``drop_last`` and ``shuffle`` as the reference sets them (data.py:516-528).

    Every ``__iter__`` draws a fresh permutation from ``self.generator``, a ``torch.Generator`` of the loader's own whose
    first seed comes from torch's default generator (so ``torch.manual_seed`` before ``get_loader`` fixes the epochs, as it
    fixes ``transforms.TorchDraws``); ``seed(n)`` sets it.  A batch is ``num_workers`` threads reading the files
    (``dataset.read_host``), one pinned buffer and one copy per task, then ``compile_transforms`` on the list of raw
    samples: the transform draws are made on the consumer's thread in sample order, so a batch depends on the
    permutation and on the draws alone.

    ``prefetch=1``: batch k + 1 is read and uploaded on a side stream while the consumer works on batch k; the consumer's
    stream waits for the upload's event before the gather, and the side stream for the gather's event before it writes
    the buffers again.  ``prefetch=0``: no thread and no second stream, everything in ``__iter__`` on the current stream.
    There are no worker processes: each would open the GPU.

    Data parallel: ``batch_size`` is the GLOBAL batch of a step, whatever the world size, so ``len()`` does not
    depend on it; rank ``rank`` of ``world`` reads ``parallel.shard_range(batch_size, world, rank)`` of every batch
    (``local_batch_size`` samples) out of ONE permutation that all ranks share.  ``rank=None, world=None``: the process
    group's when ``parallel.is_distributed()`` -- the generator's seed is then rank 0's draw, broadcast -- else 0 of 1.
    ``seed(n)`` must be called with the same ``n`` on every rank.  The transform draws stay per rank.  With
    ``LOCAL_WORLD_SIZE`` in the environment the reader threads are at most ``16 // LOCAL_WORLD_SIZE`` (one at least).

    ``decode`` (``opts.data.loaders.decode``): "host" -- the above, the default -- or "device" (a cuda device
    only): the reader threads run ``dataset.read_file``, which reads and probes a file and leaves every PNG or JPEG file the
    device decoders take, and whose array the task accepts, as a ``FileRecord``; ``_decode`` puts all of a batch's such files
    into one blob per codec and decodes them in one call (``ops.png_decode_rows`` / ``ops.png_decode``,
    ``ops.jpeg_decode``), and the decoded arrays go to ``dataset.wrap`` with nothing known of them.  Every other file, and a
    file the decoder reports as corrupt, goes through ``read_host`` as before.  The batches are the host mode's, bit for bit.
    ``decode_counts``: files since construction by who decoded them; ``times["decode"]`` exists in device mode only."""

    def __init__(self, dataset, batch_size, num_workers=0, prefetch=1, shuffle=True, device=None, transform=None,
                 rank=None, world=None, decode="host"):
        if decode not in DECODE_MODES:
            raise ValueError("OmniLoader: decode=%r; one of %s" % (decode, ", ".join(DECODE_MODES)))
        self.dataset, self.batch_size, self.decode = dataset, int(batch_size), decode
        from_group = rank is None and world is None and parallel.is_distributed()
        if from_group:
            rank, world = parallel.rank(), parallel.world()
        self.rank, self.world = int(rank or 0), int(1 if world is None else world)
        # this rank's samples of every global batch; a batch the world does not divide is refused here
        self._first, self.local_batch_size = 0, self.batch_size
        if (self.rank, self.world) != (0, 1):
            self._first, self.local_batch_size = parallel.shard_range(self.batch_size, self.world, self.rank)
        self.num_workers = max(0, min(int(num_workers), MAX_WORKERS))
        if os.environ.get("LOCAL_WORLD_SIZE"):          # the ranks of one machine share its CPUs
            self.num_workers = min(self.num_workers, max(1, MAX_WORKERS // int(os.environ["LOCAL_WORLD_SIZE"])))
        self.prefetch, self.shuffle = int(bool(prefetch)), shuffle
        self.device = torch.device(device) if device is not None else _device(dataset.device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if decode == "device" and self.device.type != "cuda":
            raise ValueError("OmniLoader: decode=\"device\" needs a cuda device, got %s" % self.device)
        self.transform = transform if transform is not None else compile_transforms(dataset.opts, dataset.mode, dataset.domain)
        self.generator = torch.Generator()
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        if from_group:
            # one permutation for all ranks: rank 0's draw (every rank still makes its own, so that torch's default
            # generator moves as it does in one process).  A loader built with an explicit rank / world takes part in no
            # collective: its caller gives the ranks one seed (``seed(n)``, or ``torch.manual_seed`` before)
            box = [seed]
            torch.distributed.broadcast_object_list(box, src=0)
            seed = int(box[0])
        self.generator.manual_seed(seed)
        self.last_order = None
        self.times = {"read": 0.0, "stage": 0.0, "transform": 0.0, "batches": 0}     # host seconds, summed
        if decode == "device":
            self.times["decode"] = 0.0                  # the part of "stage" spent on the files the device decodes
        self.decode_counts = {"png": 0, "jpeg": 0, "host": 0}      # files since construction, by who decoded them
        self._slots = [_Slot(), _Slot()]
        self._pool = self._coord = self._side = self._pending = None

    def seed(self, n):
        self.generator.manual_seed(int(n))
        return self

    def set_draws(self, draws):
        """The source of the transform draws of the batch path (default: the reference's numpy / random calls)"""
        set_draws(self.transform.transforms, draws)
        return self

    def __len__(self):
        return len(self.dataset) // self.batch_size

    # -------------------------------------------------------------------------------------------- the producer's half
    def _read(self, indices):
        t0 = time.perf_counter()
        read = self.dataset.read_file if self.decode == "device" else self.dataset.read_host
        if self._pool is not None:
            samples = list(self._pool.map(read, indices))
        else:
            samples = [read(i) for i in indices]
        self.times["read"] += time.perf_counter() - t0
        return samples

    def _stage(self, samples, slot, stream):
        """The arrays of every task into the slot's pinned buffer, one copy per task on ``stream``; returns per sample
        {task: (device array, known)}"""
        t0 = time.perf_counter()
        if slot.uploaded is not None:
            slot.uploaded.synchronize()                 # the copy that last read the pinned buffers has run
        staged = [{} for _ in samples]
        with torch.cuda.stream(stream):
            if slot.consumed is not None:
                stream.wait_event(slot.consumed)        # the gather that last read the device buffers has run
            for task in samples[0]:
                rows = [(k, s[task]) for k, s in enumerate(samples) if not isinstance(s[task], FileRecord)]
                arrays = [v[0] for _, v in rows]
                offsets, total = [], 0
                for a in arrays:
                    offsets.append(total)
                    if not torch.is_tensor(a):
                        total += (a.nbytes + _Slot.ALIGN - 1) // _Slot.ALIGN * _Slot.ALIGN
                pinned, dev = slot.buffers(task, total, self.device)
                host = pinned.numpy()
                for a, off in zip(arrays, offsets):
                    if not torch.is_tensor(a):
                        host[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
                if total:
                    dev[:total].copy_(pinned[:total], non_blocking=True)
                for (k, v), a, off in zip(rows, arrays, offsets):
                    if torch.is_tensor(a):
                        t = a.to(self.device)
                    else:
                        t = dev[off:off + a.nbytes].view(torch.from_numpy(a[:0]).dtype).view(a.shape)
                    staged[k][task] = (t, v[1])
            if self.decode == "device":
                self.decode_counts["host"] += sum(not isinstance(v, FileRecord) for s in samples for v in s.values())
                self._decode(samples, staged, slot)
                staged = [{task: st[task] for task in s} for s, st in zip(samples, staged)]     # the tasks in the list's order
            slot.uploaded = torch.cuda.Event()
            slot.uploaded.record(stream)
        self.times["stage"] += time.perf_counter() - t0
        return staged

    def _upload(self, slot, key, pieces, offsets, total):
        """``pieces`` (buffers of bytes) at ``offsets`` of the slot's pinned buffer ``key``, one copy -> the device bytes"""
        pinned, dev = slot.buffers(key, total, self.device)
        host = pinned.numpy()
        for piece, off in zip(pieces, offsets):
            b = np.frombuffer(piece, dtype=np.uint8)
            host[off:off + b.size] = b
        dev[:total].copy_(pinned[:total], non_blocking=True)
        return dev[:total]

    def _decode(self, samples, staged, slot):
        """The files the reader threads left to the device decoders (``FileRecord``), on the current stream: per codec the
        bytes of ALL tasks' files in one blob in the slot's pinned buffer, one upload each of the blob, of the descriptors and
        (PNG) of the row tables, ONE decoder call and one wait for its status words.  The decoded arrays -- views into the
        call's output, [H, W] for one channel, [H, W, C] otherwise -- go to ``staged`` with nothing known of them:
        ``RawSource`` finds min / max and the mask's threshold on the device.  A file whose status is not OK is read again by
        ``read_host`` and uploaded on its own.

        The output is allocated under this stream and read by the consumer's: the SLOT holds it (``slot.decoded``) until
        the next ``_stage`` of the slot, which drops it only behind this stream's wait for the slot's ``consumed`` event --
        the same rule that protects ``slot.dev``; no ``record_stream``."""
        t0 = time.perf_counter()
        held = []
        for codec in ("png", "jpeg"):
            todo = [(k, task, v) for k, s in enumerate(samples) for task, v in s.items()
                    if isinstance(v, FileRecord) and v.codec == codec]
            if not todo:
                continue
            descs = ((_lib.PngDesc if codec == "png" else _lib.JpegDesc) * len(todo))()
            offsets, at, out_at = [], 0, 0
            for i, (_, _, v) in enumerate(todo):
                d = v.desc
                d.blob_offset, d.out_offset = at, out_at
                offsets.append(at)
                at += -(-len(v.stream) // 16) * 16
                pixels = d.width * d.height * (d.channels * (d.bit_depth // 8) if codec == "png" else d.ncomp)
                out_at += -(-pixels // 16) * 16
                descs[i] = d
            blob = self._upload(slot, codec, [v.stream for _, _, v in todo], offsets, at)
            descs_dev = self._upload(slot, codec + "_descs", [descs], [0], C.sizeof(descs))
            if codec == "jpeg":
                out, status = ops.jpeg_decode(blob, descs, descs_dev)
            elif any(v.table is not None for _, _, v in todo):
                tables = (C.c_uint32 * sum(len(v.table) for _, _, v in todo if v.table is not None))()
                words = 0
                for _, _, v in todo:
                    if v.table is not None:
                        C.memmove(C.byref(tables, 4 * words), v.table, 4 * len(v.table))
                        words += len(v.table)
                tables_dev = self._upload(slot, "png_tables", [tables], [0], 4 * words).view(torch.int32)
                out, status, _ = ops.png_decode_rows(blob, descs, descs_dev, tables, tables_dev)
            else:
                out, status = ops.png_decode(blob, descs, descs_dev)
            held.append(out)
            view = png.image_view if codec == "png" else jpeg.image_view
            for (k, task, v), d, s in zip(todo, descs, status.tolist()):            # the one wait of this codec's call
                if s == 0:
                    img = view(out, d)
                    staged[k][task] = (img.view(d.height, d.width) if img.shape[2] == 1 else img, {})
                    self.decode_counts[codec] += 1
                else:
                    arr, known = read_host(v.path, task, self.dataset.domain)
                    staged[k][task] = ((arr if torch.is_tensor(arr) else torch.from_numpy(arr)).to(self.device), known)
                    self.decode_counts["host"] += 1
        slot.decoded = held
        self.times["decode"] += time.perf_counter() - t0

    def _prepare(self, indices, slot):
        """(reader threads ->) pinned buffers -> device, on the side stream; runs in the coordinator thread"""
        torch.cuda.set_device(self.device)
        return self._stage(self._read(indices), slot, self._side)

    def _start(self):
        if self._coord is None:
            self._coord = ThreadPoolExecutor(max_workers=1, thread_name_prefix="omni-stage")
            if self.num_workers > 0:
                self._pool = ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix="omni-read")
            self._side = torch.cuda.Stream(device=self.device)

    def _drain(self):
        """Wait for a batch that an abandoned iteration left in flight (its slot is written by another thread)"""
        pending, self._pending = self._pending, None
        if pending is not None:
            try:
                pending.result()
            except Exception:           # nobody asked for that batch
                pass

    def close(self):
        """Stop the threads (a later ``__iter__`` starts them again)"""
        self._drain()
        for pool in (self._coord, self._pool):
            if pool is not None:
                pool.shutdown(wait=True)
        self._coord = self._pool = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -------------------------------------------------------------------------------------------- the consumer's half
    def collate(self, indices, data):
        """The reference's default collate of the per-sample items (data.py:467-482)"""
        paths = [self.dataset.samples_paths[i] for i in indices]
        domain = self.dataset.domain if self.dataset.domain != "kitti" else "s"
        return {"data": data, "paths": {task: [p[task] for p in paths] for task in paths[0]},
                "domain": [domain] * len(indices), "mode": [self.dataset.mode] * len(indices)}

    def _finish(self, indices, staged, slot):
        t0 = time.perf_counter()
        stream = torch.cuda.current_stream(self.device)
        stream.wait_event(slot.uploaded)
        samples = [{task: self.dataset.wrap(task, t, known) for task, (t, known) in s.items()} for s in staged]
        data = self.transform(samples)
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(stream)
        self.times["transform"] += time.perf_counter() - t0
        self.times["batches"] += 1
        return self.collate(indices, data)

    def batches(self):
        """The index lists of one epoch: a fresh permutation (``last_order``: the whole of it, the same on every rank), cut
        into full global batches, of each of which this rank takes its ``local_batch_size`` samples -- the ranks' lists of
        step k, in rank order, are the list of a one-process loader with the same seed"""
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        self.last_order = order
        first, per = self._first, self.local_batch_size
        return [order[k * self.batch_size + first:k * self.batch_size + first + per] for k in range(len(self))]

    def __iter__(self):
        self._drain()
        batches = self.batches()
        if self.device.type != "cuda":
            # nothing is staged: the host arrays go to ``transform`` as they are.  The kernels have no CPU path, so this
            # serves a caller's own transform only (the tests of the bookkeeping)
            for indices in batches:
                yield self.collate(indices, self.transform([{t: v[0] for t, v in s.items()} for s in self._read(indices)]))
            return
        if not self.prefetch:
            slot = self._slots[0]
            for indices in batches:
                yield self._finish(indices, self._stage(self._read(indices), slot, torch.cuda.current_stream(self.device)), slot)
            return
        self._start()
        if batches:
            self._pending = self._coord.submit(self._prepare, batches[0], self._slots[0])
        for k, indices in enumerate(batches):
            staged = self._pending.result()
            self._pending = None
            if k + 1 < len(batches):        # the next batch is read and uploaded while this one is transformed and used
                self._pending = self._coord.submit(self._prepare, batches[k + 1], self._slots[(k + 1) % 2])
            yield self._finish(indices, staged, self._slots[k % 2])


def get_loader(mode, domain, opts, prefetch=1, device=None, *, rank=None, world=None):
    """reference data.py:506-528: the loader of one mode and domain; ``opts.data.loaders.batch_size`` samples per batch
    (``opts.train.kitti.batch_size`` for the kitti domain while ``train.kitti.pretrain``), shuffled, the last partial batch
    dropped, ``min(opts.data.loaders.num_workers, 16)`` reader threads.  Either batch size is the global one of a
    data-parallel run; ``rank`` / ``world`` as ``OmniLoader`` reads them."""
    loaders = opts.data.get("loaders") or {}
    decode = loaders.get("decode", "host")
    if decode not in DECODE_MODES:
        raise ValueError("get_loader: data.loaders.decode = %r; one of %s" % (decode, ", ".join(DECODE_MODES)))
    kitti = opts.train.get("kitti") or {}
    if domain != "kitti" or not kitti.get("pretrain") or not kitti.get("batch_size"):
        batch_size = loaders.get("batch_size", 4)
    else:
        batch_size = kitti.get("batch_size", 4)
    return OmniLoader(OmniListDataset(mode, domain, opts, device=device), batch_size,
                      num_workers=loaders.get("num_workers", 8), prefetch=prefetch, device=device, rank=rank, world=world,
                      decode=decode)


def loader_domains(opts):
    """The domains the tasks read, as the reference's ``load_opts`` sets ``opts.domains`` (utils.py:164-172): r and s for
    the Masker's tasks, rf for the Painter; kitti whenever it is listed (``Trainer.loaders`` leaves it out)"""
    if opts.get("domains"):
        return list(opts.domains)
    domains = ["r", "s"] if any(t in opts.tasks for t in "msd") else []
    if "p" in opts.tasks:
        domains.append("rf")
    return domains + ["kitti"]


def list_path(opts, mode, domain):
    """data.py:413-417: the file list of a mode and domain; a name without ``/`` lies in ``opts.data.files.base``"""
    path = Path(opts.data.files[mode][domain])
    return path if "/" in str(path) else Path(opts.data.files.base) / path


def listed_files(opts):
    """The file lists ``get_all_loaders`` would read, existing or not"""
    files = (opts.get("data") or {}).get("files") or {}
    return [list_path(opts, mode, domain) for mode in ("train", "val") if mode in files
            for domain in loader_domains(opts) if domain in files[mode]]


def get_all_loaders(opts, prefetch=1, device=None, *, rank=None, world=None):
    """reference data.py:531-539: ``{mode: {domain: loader}}`` for the modes and domains listed in ``opts.data.files``"""
    loaders = {}
    for mode in ["train", "val"]:
        loaders[mode] = {}
        if mode in opts.data.files:
            for domain in loader_domains(opts):
                if domain in opts.data.files[mode]:
                    loaders[mode][domain] = get_loader(mode, domain, opts, prefetch, device, rank=rank, world=world)
    return loaders
