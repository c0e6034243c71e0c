"""The training loop from file lists (climategan_amd/trainer.py: setup's loaders and display images, ``run_epoch()`` /
``run_evaluation()`` without arguments, ``train()``; ``python -m climategan_amd.train``) on the dataset
tests/loader_fixture.py writes, with the Masker configuration of tests/test_gpu_train.py (``default_opts()``, tasks d, s, m)
at 128 x 128: the fixture's transforms plus the per-task resize the decoders read their target sizes from."""
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import yaml

import loader_fixture as lf

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
ITEMS = lf.ITEMS + [{"name": "resize", "ignore": False, "new_size": {"default": 128, "d": 32, "s": 32}}]


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    root = tmp_path_factory.mktemp("loop")
    return root, lf.write(root)


def loop_opts(root, out, epochs=2):
    opts = lf.fixture_opts(root, ("d", "s", "m"), items=ITEMS)
    opts.output_path = str(out)
    opts.train.epochs = epochs
    return opts


def seed_all(n):
    random.seed(n)
    np.random.seed(n)
    torch.manual_seed(n)


def build_masker_trainer(opts, seed=66, gain=1.6):
    """tests/test_gpu_train.py's helper on these options: the filled state dicts, bf16"""
    from climategan_amd import fill
    from climategan_amd.trainer import Trainer

    seed_all(0)
    T = Trainer(opts, device="cuda").setup(inference=False)
    for mod, s in ((T.G, seed), (T.D, seed + 1)):
        shapes = {k: tuple(v.shape) for k, v in mod.state_dict().items()}
        mod.load_state_dict({k: torch.from_numpy(v) for k, v in fill.fill_state_dict(shapes, s, gain=gain).items()})
    T.G.set_compute_dtype(torch.bfloat16)
    T.D.set_compute_dtype(torch.bfloat16)
    return T


def close(T):
    for mode_dict in T.all_loaders.values():
        for loader in mode_dict.values():
            loader.close()


def test_setup_and_train_two_epochs(fixture, tmp_path):
    from climategan_amd.data import OmniLoader
    root, _ = fixture
    T = build_masker_trainer(loop_opts(root, tmp_path / "run"))
    # setup: every listed domain the tasks read, kitti only in all_loaders; two display images per mode and domain
    assert {m: list(d) for m, d in T.all_loaders.items()} == {"train": ["r", "s", "kitti"], "val": ["r", "s", "kitti"]}
    assert {m: list(d) for m, d in T.loaders.items()} == {"train": ["r", "s"], "val": ["r", "s"]}
    assert all(isinstance(ld, OmniLoader) and len(ld) == 2 and len(ld.dataset) == 5 for d in T.loaders.values() for ld in d.values())
    assert {m: {d: len(v) for d, v in dd.items()} for m, dd in T.display_images.items()} == \
        {"train": {"r": 2, "s": 2}, "val": {"r": 2, "s": 2}}
    im = T.display_images["val"]["s"][0]
    assert set(im) == {"data", "paths", "domain", "mode"} and im["data"]["x"].shape == (3, 128, 128)
    assert im["data"]["s"].shape == (1, 32, 32) and im["data"]["m"].shape == (1, 128, 128) and im["data"]["x"].is_cuda
    first = [next(iter(T.train_loaders)) for _ in range(1)][0]
    assert [b["domain"][0] for b in first] == ["r", "s"]                       # zipped in the dict's order
    lr0 = [g["lr"] for g in T.g_opt.param_groups]
    w0 = T.G.encoder.layer4[2].conv3.weight.detach().clone()
    sched0 = T.g_scheduler.last_epoch
    results = T.train()
    assert T.global_step == 2 * min(len(ld) for ld in T.loaders["train"].values()) == 4
    assert T.epoch == 2 and T.g_scheduler.last_epoch == sched0 + 2 and T.d_scheduler.last_epoch == sched0 + 2
    assert len(lr0) == len(T.g_opt.param_groups)
    assert not torch.equal(T.G.encoder.layer4[2].conv3.weight.detach(), w0)
    ckpt = tmp_path / "run" / "checkpoints" / "latest_ckpt.pth"
    assert ckpt.exists()
    saved = torch.load(ckpt, map_location="cpu", weights_only=False)
    assert saved["epoch"] == 2 and saved["step"] == 4 and {"G", "D", "g_opt", "d_opt"} <= set(saved)
    assert all(torch.isfinite(v.float()).all() for v in T.G.state_dict().values())
    assert len(results) == 2
    for res in results:
        assert set(res) == {"losses", "metrics"} and set(res["metrics"]) == {"r", "s"}
        assert len(res["losses"]) >= 8 and all(k.startswith("G.") and np.isfinite(v) for k, v in res["losses"].items())
        for tab in res["metrics"].values():
            assert set(tab) == {"m", "s"} and all(set(v) == {"accuracy", "mIOU"} for v in tab.values())
    assert T.current_mode == "train"
    close(T)


def test_run_epoch_from_the_loaders_equals_run_epoch_on_their_batches(fixture, tmp_path):
    """two fresh, identically seeded trainers: one reads its loaders, the other is handed the batches an identically seeded
    pass over its own loaders produced; the parameters after the epoch are bit-identical (the step is deterministic:
    tests/test_gpu_determinism.py)"""
    from climategan_amd import ops
    root, _ = fixture
    trainers = [build_masker_trainer(loop_opts(root, tmp_path / ("run%d" % k))) for k in range(2)]
    sd_g = {k: v.clone() for k, v in trainers[0].G.state_dict().items()}
    sd_d = {k: v.clone() for k, v in trainers[0].D.state_dict().items()}

    def reset(T):
        T.G.load_state_dict(sd_g)
        T.D.load_state_dict(sd_d)
        ops.touch(*T.G.parameters(), *T.G.buffers(), *T.D.parameters(), *T.D.buffers())
        for ld in T.loaders["train"].values():
            ld.seed(11)
        seed_all(7)

    A, B = trainers
    reset(A)
    last_a = A.run_epoch()
    reset(B)
    B.train_mode()
    batches = list(B._multi_domain_batches(B.train_loaders, True))
    assert len(batches) == 2 and all(set(b) == {"r", "s"} for b in batches)
    seed_all(7)
    last_b = B.run_epoch(batches)
    torch.cuda.synchronize()
    assert A.global_step == B.global_step == 2 and A.epoch == B.epoch == 1
    assert float(last_a[0]) == float(last_b[0]) and float(last_a[1]) == float(last_b[1])
    for name, a, b in (("G", A.G, B.G), ("D", A.D, B.D)):
        sa, sb = a.state_dict(), b.state_dict()
        bad = [k for k in sa if not torch.equal(sa[k], sb[k])]
        assert not bad, (name, len(bad), bad[:5])
    assert any(not torch.equal(v, sd_g[k]) for k, v in A.G.state_dict().items() if v.is_floating_point())
    close(A)
    close(B)


def test_unbuilt_schedules_are_refused_at_setup(fixture, tmp_path):
    from climategan_amd.trainer import Trainer
    root, _ = fixture
    opts = loop_opts(root, tmp_path)
    opts.train.kitti.pretrain = True
    with pytest.raises(NotImplementedError, match="train.kitti.pretrain"):
        Trainer(opts, device="cuda").setup()
    opts = loop_opts(root, tmp_path)
    opts.train.pseudo.tasks = ["d"]
    with pytest.raises(NotImplementedError, match="train.pseudo.tasks"):
        Trainer(opts, device="cuda").setup()
    opts.train.pseudo.epochs = 0                 # pseudo-label training switched off by its epoch count: not refused
    Trainer(opts, device="cuda")._refuse_unbuilt_training_options()
    with pytest.raises(ValueError, match="no train loaders"):
        from climategan_amd.config import default_opts
        plain = default_opts()
        plain.tasks = ["d", "s", "m"]
        T = Trainer(plain, device="cuda")
        T.loaders = None
        T.train_loaders


def test_cli_trains_an_epoch_and_the_run_resumes(fixture, tmp_path):
    from climategan_amd import train
    from climategan_amd.trainer import Trainer
    root, _ = fixture
    run = tmp_path / "cli_run"
    cfg = tmp_path / "cfg.yaml"
    opts = loop_opts(root, run, epochs=1)
    cfg.write_text(yaml.safe_dump({k: train.plain(opts[k]) for k in ("tasks", "data", "comet")}))
    cmd = [sys.executable, "-m", "climategan_amd.train", "--config", str(cfg), "--output", str(run), "train.epochs=1",
           "train.fid.n_images=3"]
    done = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-2000:]
    assert "epoch 0: 2 steps" in done.stdout
    assert (run / "opts.yaml").exists() and (run / "checkpoints" / "latest_ckpt.pth").exists()
    written = yaml.safe_load((run / "opts.yaml").read_text())
    assert written["train"]["epochs"] == 1 and written["output_path"] == str(run) and written["tasks"] == ["d", "s", "m"]
    T = Trainer.resume_from_path(run, inference=False, device="cuda", verbose=0)
    assert T.epoch == 1 and T.global_step == 2 and T.opts.train.resume is True
    assert len(T.loaders["train"]["r"]) == 2 and len(T.display_images["val"]["r"]) == 2
    saved = torch.load(run / "checkpoints" / "latest_ckpt.pth", map_location="cuda", weights_only=False)
    assert all(torch.equal(v, saved["G"][k]) for k, v in T.G.state_dict().items())
    close(T)
