"""Write tests/golden/data_transforms.npz by running the REAL reference's loader transforms (climategan/transforms.py:22-289,
424-490) on the CPU (dev container only; TEST INFRASTRUCTURE, like tests/devtools/make_golden_diffaug.py).

    python tests/devtools/make_golden_data_transforms.py          # from the repo root, needs the reference tree

The cases and their inputs live in tests/data_transform_cases.py (inputs from climategan_amd.fill: only outputs are stored).

What is NOT the reference's own code here, and why:
  * ``torchvision`` is not installed, so oracle.ref_shim stubs it and the reference's ``Normalize`` would hold an object that
    cannot be called.  ``trsfs.Normalize`` INSIDE THE IMPORTED REFERENCE MODULE is replaced by ``_Normalize`` below: the three
    lines ``(t - mean) / std`` with fp32 [C, 1, 1] constants, which is what torchvision's ``Normalize`` computes.  The
    reference hands the HRNet constants over as ONE argument ``((mean), (std))`` (transforms.py:217-219), which torchvision's
    constructor would refuse; the stand-in unpacks it, so the HRNet case pins the constants the reference names.
  * The reference module's ``np`` and ``random`` are proxies that record the results of ``np.random.rand``,
    ``np.random.randint`` and ``random.uniform`` in call order; the tests replay them
    (climategan_amd.transforms.RecordedPipelineDraws) or check that the mirror's default draw source, seeded the same way,
    reproduces them.
  * ``F.interpolate(mode="nearest")`` has no int64 kernel on the CPU of the installed torch.  The case ``int64_s`` therefore
    runs the reference on the fp32 tensor that holds the same class ids (0..10, exact in fp32) and stores the result as
    int64: a nearest resize, a crop and a flip only move elements, so the element type cannot change which ones they move.
  * The colour-jitter classes call torchvision's ``adjust_*``: the fixture records that ``get_transforms`` returns them (the
    class lists), never their output; the tests pin them to torchvision's documented formulas instead.
"""
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import data_transform_cases as dc  # noqa: E402
from oracle import ref_shim  # noqa: E402
from oracle.make_golden import GOLDEN_DIR  # noqa: E402


class _Normalize:
    def __init__(self, mean, std=None):
        mean, std = (mean, std) if std is not None else mean
        self.mean, self.std = (torch.tensor(v, dtype=torch.float32).view(-1, 1, 1) for v in (mean, std))

    def __call__(self, t):
        return (t - self.mean) / self.std


class _Recorder:
    """``np`` / ``random`` for the reference's transforms module: everything passes through, the three draws are recorded"""

    def __init__(self, real, log, sub=None):
        self._real, self._log = real, log
        if sub:
            self.random = _Recorder(getattr(real, sub), log)

    def __getattr__(self, k):
        return getattr(self._real, k)

    def _rec(self, kind, v):
        self._log.append((kind, float(v)))
        return v

    def rand(self, *a):
        return self._rec("rand", self._real.rand(*a))

    def randint(self, *a, **k):
        return self._rec("randint", self._real.randint(*a, **k))

    def uniform(self, *a):
        return self._rec("uniform", self._real.uniform(*a))


def reference_module():
    import random

    tr = ref_shim.ref("transforms")
    tr.trsfs.Normalize = _Normalize
    log = []
    tr.np = _Recorder(np, log, "random")
    tr.random = _Recorder(random, log)
    return tr, log


def first_flip(seed):
    dc.seed_all(seed)
    return not (np.random.rand() > 0.5)


def run_case(tr, log, name, case):
    seed = case["seed"]
    if seed is None:
        seed = next(s for s in range(100, 1000) if first_flip(s) == case["want_flip"])
    opts = ref_shim.Dict(dc.case_opts(case))
    transforms = tr.get_transforms(opts, case["mode"], case.get("domain", "r"))
    out = {name + ".seed": np.array([seed], dtype=np.int64),
           name + ".classes": np.array([type(t).__name__ for t in transforms])}
    del log[:]
    dc.seed_all(seed)
    for k, shapes in enumerate(case["samples"]):
        data = {task: torch.from_numpy(v) for task, v in dc.sample_inputs(name, k, shapes).items()}   # s as fp32: see above
        for t in transforms:
            data = t(data)
        for task, v in data.items():
            v = v.numpy()
            if task == "s" and case.get("s_int64"):
                v = v.astype(np.int64)
            out["%s.%d.%s" % (name, k, task)] = dc.subsample(v, case.get("sub"))
    out[name + ".draw_kinds"] = np.array([k for k, _ in log] or [""])[:len(log)]
    out[name + ".draw_values"] = np.array([v for _, v in log], dtype=np.float64)
    return out


def main():
    if not ref_shim.available():
        sys.exit("make_golden_data_transforms needs the reference tree (dev container only)")
    torch.set_num_threads(8)
    tr, log = reference_module()
    ref_items = ref_shim.default_opts().data.transforms
    assert [dict(i) for i in ref_items] == dc.DEFAULT_ITEMS, "DEFAULT_ITEMS no longer restates defaults.yaml:43-67"
    out = {}
    for name, case in dc.CASES.items():
        out.update(run_case(tr, log, name, case))
        print("%-20s %s" % (name, " ".join(out[name + ".classes"])))
    # the class lists of the default item list, with and without the Painter task
    for mode in ("train", "val"):
        for tag, tasks in (("p", ["d", "s", "m", "p"]), ("nop", ["d", "s", "m"])):
            opts = ref_shim.Dict(dc.case_opts(dc.CASES["default_640"], tasks))
            out["classes.%s.%s" % (mode, tag)] = np.array([type(t).__name__ for t in tr.get_transforms(opts, mode, "r")])
    r = tr.Resize(640, keep_aspect_ratio=True)
    out["new_size"] = np.array([r.compute_new_default_size(torch.empty(1, 1, h, w)) for h, w in dc.NEW_SIZE_SHAPES],
                               dtype=np.int64)
    path = GOLDEN_DIR / "data_transforms.npz"
    np.savez_compressed(path, **out)
    print("%s: %d B, %d arrays" % (path.name, path.stat().st_size, len(out)))
    assert path.stat().st_size < 2 ** 20


if __name__ == "__main__":
    main()
