"""Write tests/golden/display_indices.json by calling the REAL reference's ``get_display_indices`` (climategan/utils.py:669-713;
dev container only; TEST INFRASTRUCTURE, like make_golden_data_decode.py).

    python tests/devtools/make_golden_display_indices.py          # from the repo root, needs the reference tree

Only the cases (display size, fid images, domain, dataset length) and the indices the reference returns are stored.  A list
as display size is not a case: the reference compares it with the dataset's length and fails (utils.py:694)."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from oracle import ref_shim  # noqa: E402
from oracle.make_golden import GOLDEN_DIR  # noqa: E402

CASES = [dict(display_size=d, n_images=f, domain=dom, length=n)
         for d, f, dom, n in [(20, 57, "r", 100), (20, 57, "s", 1000), (20, 57, "rf", 57), (20, 57, "rf", 300), (2, 0, "r", 5),
                              (2, 0, "s", 5), (2, 3, "rf", 5), (8, 0, "r", 5), (0, 0, "s", 7), (5, 0, "kitti", 12)]]


def main():
    utils = ref_shim.ref("utils")
    out = []
    for case in CASES:
        opts = ref_shim.Dict({"comet": {"display_size": case["display_size"]}, "train": {"fid": {"n_images": case["n_images"]}}})
        np.random.seed(5)
        before = np.random.get_state()[1].copy()
        indices = [int(i) for i in utils.get_display_indices(opts, case["domain"], case["length"])]
        assert np.array_equal(before, np.random.get_state()[1])
        out.append(dict(case, indices=indices))
    path = GOLDEN_DIR / "display_indices.json"
    path.write_text(json.dumps(out, indent=1) + "\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    main()
