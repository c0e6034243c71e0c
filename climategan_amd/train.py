"""Mirror of the reference's ``train.py`` (:36-183) without hydra, comet and the SLURM auto-resume: options in, a trained
run directory out.

    python -m climategan_amd.train [--config FILE.yaml] [--resume RUN_DIR] [--output RUN_DIR] [--dtype bf16|fp16]
                                   [--backend nccl|gloo] [--dist-timeout SECONDS] [--seed N] [key.sub=value ...]

Data parallel, one process per GPU -- the program goes after the launcher's own options, and the launcher
starts every rank as a fresh process:

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m climategan_amd.train --config FILE.yaml

``main()`` reads the launcher's environment (``parallel.init_from_env``: ``RANK``, ``WORLD_SIZE``, ``LOCAL_RANK``,
``MASTER_ADDR``, ``MASTER_PORT``; without ``WORLD_SIZE`` this is one process and none of the following applies).
``data.loaders.batch_size`` is the GLOBAL batch per domain and step, of which every rank reads its equal share, so the
steps per epoch, the schedulers and ``global_step`` do not depend on the number of GPUs.  Rank 0 alone creates the run
directory, writes ``opts.yaml`` and the checkpoints and prints the tables; ``--resume`` reads the same file on every
rank.  ``--seed N`` seeds ``random``, numpy and torch with ``N`` before the setup on every rank (the same initial model)
and with ``N + 1 + rank`` after it (augmentation draws and label noise differ across ranks, reproducibly).

The options are ``config.default_opts()`` with the loop's part of ``shared/trainer/defaults.yaml`` (``train_defaults``),
then the ``--config`` file, then the dotted overrides, whose values are read by ``yaml.safe_load`` (``train.epochs=2``,
``tasks=[d,s,m]``, ``data.files.base=/data/lists``).  ``opts.yaml`` is written into the run directory
(``opts.output_path``, or ``--output``), where ``Trainer.resume_from_path`` looks for it; then ``Trainer(opts).setup()``
and ``train()``.  ``--resume RUN_DIR`` continues that run through ``Trainer.resume_from_path(RUN_DIR, inference=False)``,
with the overrides merged over its ``opts.yaml``.

Keys that only the reference's launcher understands are refused by name (``REFUSED``) instead of being ignored.
"""
import argparse
import sys
from pathlib import Path

import yaml

from .config import Opts, default_opts

# key prefix -> why it is refused, in the style of apply_events.REFUSED.  ``comet.display_size`` is the one comet key the
# loop reads (``utils.get_display_indices``: how many display images ``eval_images`` scores).
REFUSED = {
    "comet": "comet logging: this launcher does not log to comet (only comet.display_size is read)",
    "hydra": "hydra launcher settings: this launcher reads one yaml file and dotted overrides",
    "defaults": "hydra config groups: this launcher reads one yaml file and dotted overrides",
    "jobs": "SLURM job lists: this launcher runs one training in this process",
    "experiment": "hydra experiment groups: this launcher reads one yaml file and dotted overrides",
    "train.auto_resume": "SLURM auto-resume: use --resume RUN_DIR",
}
ALLOWED = ("comet.display_size",)
DTYPES = ("bf16", "fp16")
BACKENDS = ("nccl", "gloo")


def train_defaults():
    """The part of shared/trainer/defaults.yaml that the loaders and the loop read (line numbers of that file), over
    ``default_opts()``.  The file lists have no default: the reference's are paths of its authors' cluster."""
    opts = default_opts()
    # data.loaders.decode ("host" | "device") is read by get_loader and is deliberately not listed: an absent key
    # means "host", and the loaders' dictionary stays the reference's two entries
    _merge_into(opts, {
        "data": {"max_samples": -1, "check_samples": False, "loaders": {"batch_size": 6, "num_workers": 6},   # :25, 38-41
                 "normalization": "default",                                                                  # :42
                 "transforms": [                                                                              # :43-67
                     {"name": "hflip", "ignore": "val", "p": 0.5},
                     {"name": "resize", "ignore": False, "new_size": 640, "keep_aspect_ratio": True},
                     {"name": "crop", "ignore": False, "center": "val", "height": 600, "width": 600},
                     {"name": "brightness", "ignore": "val"}, {"name": "saturation", "ignore": "val"},
                     {"name": "contrast", "ignore": "val"},
                     {"name": "resize", "ignore": False, "new_size": {"default": 640, "d": 160, "s": 160}}]},
        "train": {"kitti": {"pretrain": False, "epochs": 10, "batch_size": 6},                               # :264-267
                  "pseudo": {"tasks": [], "epochs": 10}, "epochs": 300, "fid": {"n_images": 57}},             # :269-274
        "comet": {"display_size": 20},                                                                        # :328
    })
    return opts


def _merge_into(destination, source):
    """Recursive dict merge: ``source``'s entries overwrite ``destination``'s (lists are replaced whole)"""
    for key, value in source.items():
        if isinstance(value, dict) and isinstance(destination.get(key), dict):
            _merge_into(destination[key], value)
        else:
            destination[key] = value
    return destination


def refuse(key):
    """SystemExit naming ``key`` when it is, or lies under, a refused key"""
    if key in ALLOWED:
        return
    for prefix, why in REFUSED.items():
        if key == prefix or key.startswith(prefix + "."):
            raise SystemExit("train: %s is not supported here: %s" % (key, why))


def _flat_keys(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, dict) and v:
            yield from _flat_keys(v, prefix + str(k) + ".")
        else:
            yield prefix + str(k)


def parse_override(arg):
    """``key.sub=value`` -> (["key", "sub"], yaml value)"""
    if "=" not in arg or arg.startswith("="):
        raise SystemExit("train: override %r is not key.sub=value" % arg)
    key, value = arg.split("=", 1)
    key = key.lstrip("+")                    # hydra's "append" prefix means nothing more here
    refuse(key)
    return key.split("."), yaml.safe_load(value)


def nest(keys, value):
    for k in reversed(keys):
        value = {k: value}
    return value


def build_opts(config=None, overrides=(), base=None):
    """defaults (or ``base``) <- the yaml file ``config`` <- dotted ``overrides``; refused keys raise SystemExit"""
    opts = base if base is not None else train_defaults()
    if config is not None:
        loaded = yaml.safe_load(Path(config).read_text()) or {}
        if not isinstance(loaded, dict):
            raise SystemExit("train: %s does not hold a mapping of options" % config)
        for key in _flat_keys(loaded):
            refuse(key)
        _merge_into(opts, loaded)
    for arg in overrides:
        keys, value = parse_override(arg)
        _merge_into(opts, nest(keys, value))
    return Opts(opts)


def plain(value):
    """Opts / tuples -> plain dicts and lists, for yaml.safe_dump"""
    if isinstance(value, dict):
        return {k: plain(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [plain(v) for v in value]
    return value


def parse_args(argv=None):
    parser = argparse.ArgumentParser(prog="python -m climategan_amd.train", description=__doc__.split("\n")[0],
                                     allow_abbrev=False)
    parser.add_argument("--config", default=None, help="yaml file of options merged over the defaults")
    parser.add_argument("--resume", default=None, metavar="RUN_DIR",
                        help="continue the run of this directory (its opts.yaml and checkpoints/latest_ckpt.pth)")
    parser.add_argument("--output", default=None, metavar="RUN_DIR", help="the run directory (sets output_path)")
    parser.add_argument("--dtype", default=None, choices=DTYPES,
                        help="the kernels' 16-bit type (default: bf16, or fp16 with train.amp)")
    parser.add_argument("--backend", default="nccl", choices=BACKENDS,
                        help="the process group's backend in a data-parallel run (nccl is RCCL on ROCm)")
    parser.add_argument("--dist-timeout", default=None, type=float, metavar="SECONDS",
                        help="the process group's timeout (default: torch's own)")
    parser.add_argument("--seed", default=None, type=int, metavar="N",
                        help="seed random, numpy and torch: N before the setup on every rank, N + 1 + rank after it")
    parser.add_argument("overrides", nargs="*", metavar="key.sub=value", help="dotted overrides, values in yaml syntax")
    args = parser.parse_args(argv)
    for arg in args.overrides:
        parse_override(arg)                 # refusals and syntax before anything is built
    return args


def seed_everything(n):
    """``random``, numpy's and torch's global generators (torch's: the host's and every GPU's)"""
    import random

    import numpy as np
    import torch
    random.seed(n)
    np.random.seed(n)
    torch.manual_seed(n)


def main(argv=None):
    args = parse_args(argv)
    import torch

    from . import parallel
    from .trainer import Trainer

    rank, _world = parallel.init_from_env(args.backend, args.dist_timeout)
    trainer = None
    try:
        if args.seed is not None:           # the same initial model and the same permutations on every rank
            seed_everything(args.seed)
        device = torch.device("cuda", torch.cuda.current_device()) if parallel.world() > 1 else None
        if args.resume is not None:
            overrides = build_opts(args.config, args.overrides, base={})
            if args.output is not None:
                overrides["output_path"] = str(args.output)
            trainer = Trainer.resume_from_path(args.resume, overrides=plain(overrides), inference=False, device=device)
            opts = trainer.opts
        else:
            opts = build_opts(args.config, args.overrides)
            if args.output is not None:
                opts.output_path = str(args.output)
            if not (opts.get("data") or {}).get("files"):
                raise SystemExit("train: no file lists -- set data.files.base and data.files.train / val (--config or overrides)")
            if parallel.is_main():          # the run directory and its opts.yaml are rank 0's; nobody reads them early
                run_dir = Path(opts.output_path)
                run_dir.mkdir(parents=True, exist_ok=True)
                (run_dir / "opts.yaml").write_text(yaml.safe_dump(plain(opts)))
            parallel.barrier()
            trainer = Trainer(opts, device=device).setup()
        if args.seed is not None:           # augmentation draws and label noise: different per rank, reproducible
            seed_everything(args.seed + 1 + rank)
        if args.dtype is not None:
            dtype = {"bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
            trainer.G.set_compute_dtype(dtype)
            trainer.D.set_compute_dtype(dtype)
        if parallel.is_main():
            print("train: %d epochs into %s" % (int(opts.train.epochs), opts.output_path))
        trainer.train()
    finally:
        if trainer is not None:
            for mode_dict in (trainer.all_loaders or {}).values():
                for loader in mode_dict.values():
                    loader.close()
        parallel.shutdown()
    return 0


if __name__ == "__main__":
    sys.exit(main())
