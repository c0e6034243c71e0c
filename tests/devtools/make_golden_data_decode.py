"""Write tests/golden/data_decode.npz by running the REAL reference's loader decode (climategan/data.py:91-148, 231-252,
344-399; tutils.py:195-293) on the CPU (dev container only; TEST INFRASTRUCTURE, like make_golden_data_transforms.py).

    python tests/devtools/make_golden_data_decode.py          # from the repo root, needs the reference tree

The cases and their raw sources live in tests/data_decode_cases.py (sources from climategan_amd.fill: only outputs are stored).

What is NOT the reference's own code here, and why:
  * ``tensor_loader`` reads files.  Every source is written as ``.npy`` into a temporary directory and read back by the
    reference's own ``np.load`` branches; ``imageio`` is not installed, so ``imread`` INSIDE THE IMPORTED REFERENCE MODULE
    is ``np.load`` (process_kitti_seg's one read).
  * Sim / real segmentation maps are ``.pt`` files made offline by ``save_segmap_tensors`` ->
    ``transform_segmap_image_to_tensor`` (data.py:274-283), which opens an image with PIL.  The script runs its three other
    lines on the array: ``encode_segmap`` (the reference's), ``torch.from_numpy(arr).float()``, ``unsqueeze(0)``.
  * The end-to-end cases run the reference's ``get_transforms`` exactly as make_golden_data_transforms.py sets it up (its
    ``Normalize`` stand-in and draw recorder are imported from there).
"""
import sys
import tempfile
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tests" / "devtools"))

import data_decode_cases as cases  # noqa: E402
import data_transform_cases as dc  # noqa: E402
from make_golden_data_transforms import reference_module  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import GOLDEN_DIR  # noqa: E402


def load_reference(data, tmp, name, task, domain, source, opts):
    """the reference's [1, C, H, W] tensor of one raw source"""
    if task == "s" and domain != "kitti":
        arr = data.encode_segmap(source, domain)                # data.py:279-283 without the PIL read
        path = tmp / (name + ".pt")
        torch.save(torch.from_numpy(arr).float().unsqueeze(0), path)
    else:
        path = tmp / (name + ".npy")
        np.save(path, source)
    return data.tensor_loader(path, task, domain, ref_shim.Dict(opts))


def main():
    if not ref_shim.available():
        sys.exit("make_golden_data_decode needs the reference tree (dev container only)")
    torch.set_num_threads(8)
    data = ref_shim.ref("data")
    data.imread = np.load
    out = {}
    for domain, table in data.classes_dict.items():
        out["classes.%s.keys" % domain] = np.array(list(table), dtype=np.int64)
        out["classes.%s.colours" % domain] = np.array(list(table.values()), dtype=np.int64)
    out["kitti_mapping"] = np.array(list(data.kitti_mapping.items()), dtype=np.int64)
    with tempfile.TemporaryDirectory() as tmp, np.errstate(all="ignore"):
        tmp = Path(tmp)
        for name, (task, domain, build, o) in cases.single_cases(data.classes_dict).items():
            ref = load_reference(data, tmp, name, task, domain, build(), cases.loader_opts(**o))
            out[name] = ref.numpy()
            print("%-18s %s %s" % (name, tuple(ref.shape), ref.dtype))
        tr, log = reference_module()
        for name, case in cases.E2E.items():
            opts = cases.e2e_opts(case)
            transforms = tr.get_transforms(ref_shim.Dict(opts), case["mode"], case["domain"])
            del log[:]
            dc.seed_all(case["seed"])
            for k, hw in enumerate(case["samples"]):
                sources = cases.e2e_sources(name, k, hw, data.classes_dict)
                sample = {task: load_reference(data, tmp, "%s.%d.%s" % (name, k, task), task, case["domain"], sources[task], opts)
                          for task in cases.E2E_TASKS}
                out["%s.%d.d_loaded" % (name, k)] = sample["d"].numpy()
                for t in transforms:
                    sample = t(sample)
                for task, v in sample.items():
                    out["%s.%d.%s" % (name, k, task)] = v.numpy()
            out[name + ".draw_kinds"] = np.array([k for k, _ in log])
            out[name + ".draw_values"] = np.array([v for _, v in log], dtype=np.float64)
            print("%-18s %d draws" % (name, len(log)))
    path = GOLDEN_DIR / "data_decode.npz"
    np.savez_compressed(path, **out)
    print("%s: %d B, %d arrays" % (path.name, path.stat().st_size, len(out)))
    assert path.stat().st_size < 2 ** 20


if __name__ == "__main__":
    main()
