"""The helpers of the reference's ``climategan/utils.py`` that the hot path needs."""


def find_target_size(opts, task):
    """reference utils.py:984-995: final ``resize`` transform's new_size for ``task`` (int or per-task dict)."""
    try:
        new_size = opts.data.transforms[-1].new_size
    except (AttributeError, KeyError, IndexError, TypeError):
        return None
    if isinstance(new_size, int):
        return new_size
    if not new_size:
        return None
    if task in new_size:
        return new_size[task]
    assert "default" in new_size
    return new_size["default"]


def flatten_opts(opts) -> dict:
    """reference utils.py:385-427: a nested dict -> one level, keys joined by '.'; lists of dicts are indexed (``a.0.b``),
    other lists become their ``str``; how ``Trainer.eval_images`` prints / logs its metric table (trainer.py:1791-1797)."""
    from pathlib import Path

    out = {}

    def walk(d, prefix):
        for k, v in d.items():
            if isinstance(v, dict):
                walk(v, prefix + str(k) + ".")
            elif isinstance(v, list):
                if v and isinstance(v[0], dict):
                    for i, m in enumerate(v):
                        walk(m, prefix + str(k) + "." + str(i) + ".")
                else:
                    out[prefix + str(k)] = str(v)
            else:
                out[prefix + str(k)] = str(v) if isinstance(v, Path) else v

    walk(opts, "")
    return out


def env_to_path(path):
    """reference utils.py:367-382: every ``/``-separated part of ``path`` that holds a ``$`` becomes the value of that
    environment variable (``$HOME/clouds`` -> ``/home/me/clouds``); a variable that is not set is a KeyError."""
    import os

    return "/".join(os.environ[el.replace("$", "")] if "$" in el else el for el in str(path).split("/"))


def get_display_indices(opts, domain, length):
    """reference utils.py:669-713: the dataset indices of the display images.  ``opts.comet.display_size`` as an int n gives
    the first n entries of ``np.random.permutation(length)`` under the temporary numpy seed 123 (the global numpy state
    is left as it was); for ``rf`` n is at least ``train.fid.n_images``.  A list is returned as it is."""
    import numpy as np

    if domain == "rf":
        dsize = max([opts.comet.display_size, opts.train.fid.get("n_images", 0)])
    else:
        dsize = opts.comet.display_size
    assert isinstance(dsize, (int, list)) and not isinstance(dsize, dict), "Unknown display size {}".format(dsize)
    if isinstance(dsize, list):
        display_indices = list(dsize)
    else:
        if dsize > length:
            print("Warning: dataset is smaller ({} images) than required display indices ({}). Selecting {} images."
                  .format(length, dsize, length))
        assert dsize >= 0, "Display size cannot be < 0"
        state = np.random.get_state()                                   # temp_np_seed, utils.py:648-666
        np.random.seed(123)
        try:
            display_indices = list(np.random.permutation(length)[:dsize])
        finally:
            np.random.set_state(state)
    if not display_indices:
        print("Warning: no display indices (utils.get_display_indices)")
    return display_indices
