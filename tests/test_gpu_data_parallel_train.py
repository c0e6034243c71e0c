"""The data-parallel train command on ONE GPU: rank-sharded loaders -> ``Trainer.train()`` -> sharded evaluation
-> rank 0's checkpoint -> ``python -m climategan_amd.train``.

Two ranks share the device, so their group is gloo (RCCL refuses two ranks on one device), as in
tests/test_gpu_two_rank.py; both get ``LOCAL_RANK=0``.  The configuration is tests/test_gpu_train_loop.py's: the Masker
(tasks d, s, m) at 128 x 128 on tests/loader_fixture.py's dataset, whose global batch of 2 leaves one sample per domain
and rank; an epoch is two steps, one ExtraAdam extrapolation and one update.  The last test runs the command on a ONE-rank
RCCL group: the only RCCL execution the command's code gets here.  Every equality is exact: each follows from
construction or from the step's determinism (tests/test_gpu_determinism.py).

Measured on one MI355X (wall time of each test): see the figures in the tests' docstrings.

Every child is a fresh process under a time limit; a child that times out or dies of a signal ends the test, kills its
sibling and makes the remaining multi-process tests of this file skip (``_BROKEN``): nothing is started on a GPU that a
sibling has just faulted, and nothing is retried."""
import contextlib
import io
import os
import socket
import subprocess
import sys
import time
from pathlib import Path

import pytest
import torch
import yaml

import loader_fixture as lf
from test_gpu_train_loop import build_masker_trainer, close, loop_opts, seed_all

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
WORKER_TIMEOUT_S, JOIN_TIMEOUT_S = 900, 120          # tests/test_gpu_two_rank.py
CLI_TIMEOUT_S = 240                                   # test_cli_trains_an_epoch_and_the_run_resumes
FATAL = (134, 139, 124, 137, -6, -11, -9)
_BROKEN = []                                          # why the multi-process tests after a dead child do not run


def _needs_healthy_children():
    if _BROKEN:
        pytest.skip("an earlier multi-process test of this file lost a child: " + _BROKEN[0])


def _free_port():
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _tensors(value, prefix=""):
    """{dotted key: tensor} of a checkpoint entry (state dicts, optimizer states)"""
    if torch.is_tensor(value):
        return {prefix: value}
    out = {}
    if isinstance(value, dict):
        for k, v in value.items():
            out.update(_tensors(v, "%s.%s" % (prefix, k)))
    elif isinstance(value, (list, tuple)):
        for k, v in enumerate(value):
            out.update(_tensors(v, "%s.%d" % (prefix, k)))
    return out


# ---- 1, 2: train() on two ranks --------------------------------------------------------------------------------------
def _tables_of(T):
    """``eval_images``' tables of a trainer, in a fixed order of calls (every forward of the mask decoder moves its
    spectral-norm vectors, so the order is part of the model's state): val r, val s, then val r with its first image only"""
    T.eval_mode()
    tables = []
    with contextlib.redirect_stdout(io.StringIO()):
        for d in ("r", "s"):
            T.eval_images("val", d)
            tables.append(T.last_metrics[("val", d)])
        every = T.display_images["val"]["r"]
        T.display_images["val"]["r"] = every[:1]
        T.eval_images("val", "r")
        tables.append(T.last_metrics[("val", "r")])
        T.display_images["val"]["r"] = every
    T.train_mode()
    return tables


def _worker(rank, world, port, root, run, q):
    try:
        sys.path.insert(0, str(ROOT))
        sys.path.insert(0, str(ROOT / "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                          LOCAL_RANK="0")
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from climategan_amd import parallel

        T = build_masker_trainer(loop_opts(root, run, epochs=1))
        assert T.g_reducer is not None and T.g_reducer.active and T.g_reducer.world == 2
        out = {"loaders": {m: {d: (ld.rank, ld.world, ld.batch_size, ld.local_batch_size, ld.num_workers, len(ld))
                               for d, ld in md.items()} for m, md in T.loaders.items()}}

        def digest(mod, what):
            ts = {"p": dict(mod.named_parameters()), "b": dict(mod.named_buffers())}[what]
            if not ts:
                return None
            v = torch.stack([t.detach().double().sum() + t.detach().double().abs().sum() * 1e-3 for t in ts.values()]).cpu()
            both = [torch.empty_like(v) for _ in range(world)]          # (gloo gathers host tensors only)
            dist.all_gather(both, v)
            return int((both[0] != both[1]).sum()), len(ts)

        seed_all(7 + rank)                                # the ranks' augmentation draws and label noise differ
        T.run_epoch()
        out["orders"] = {d: ld.last_order for d, ld in T.loaders["train"].items()}
        out["after_epoch"] = {"G.p": digest(T.G, "p"), "D.p": digest(T.D, "p"), "G.b": digest(T.G, "b")}
        parallel.broadcast_buffers(T.G)
        parallel.broadcast_buffers(T.D)
        out["after_broadcast"] = {"G.b": digest(T.G, "b"), "D.b": digest(T.D, "b")}

        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            results = T.train()                           # opts.train.epochs = 1: one more epoch
        torch.cuda.synchronize()
        out["stdout"] = printed.getvalue()
        out["counters"] = (T.global_step, T.epoch, T.current_mode)
        out["results"] = results
        out["last_metrics"] = {"%s_%s" % k: v for k, v in T.last_metrics.items()}
        parallel.barrier()
        saved = torch.load(Path(run) / "checkpoints" / "latest_ckpt.pth", map_location="cuda", weights_only=False)
        out["ckpt"] = (saved["epoch"], saved["step"], sorted(saved))
        state = T.G.state_dict()
        out["ckpt_G_differs"] = [k for k in state if not torch.equal(state[k], saved["G"][k])]
        out["ckpt_G_keys"] = (len(state), len(saved["G"]))
        state = T.D.state_dict()
        out["ckpt_D_differs"] = [k for k in state if not torch.equal(state[k], saved["D"][k])]
        # the model IS the checkpoint now: its tables, for the one-process comparison -- all display images, then a single
        # one, of which rank 1 has no share
        del saved, state
        out["ckpt_tables"] = _tables_of(T)
        out["after_eval"] = digest(T.G, "p")
        close(T)
        q.put((rank, "ok", out))
        parallel.barrier()
        parallel.shutdown()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    root = tmp_path_factory.mktemp("dp_train")
    lf.write(root)
    return root


@pytest.fixture(scope="module")
def two_rank_run(fixture, tmp_path_factory):
    """One pair of spawned ranks: an epoch by hand, the buffer broadcast, then ``train()`` for one more epoch.  Returns
    (run directory, [rank 0's report, rank 1's report], wall seconds)."""
    _needs_healthy_children()
    import queue

    import torch.multiprocessing as mp
    run = tmp_path_factory.mktemp("dp_run") / "run"
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    start = time.perf_counter()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, fixture, run, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = []
    try:
        deadline = time.monotonic() + WORKER_TIMEOUT_S
        while len(res) < len(procs):
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                if dead or time.monotonic() > deadline:
                    _BROKEN.append("two-rank train(): exit codes %s, %d of 2 reports" % ([p.exitcode for p in procs], len(res)))
                    break
        if not _BROKEN:
            for p in procs:
                p.join(timeout=JOIN_TIMEOUT_S)
    finally:
        for p in procs:
            if p.is_alive():
                _BROKEN.append("two-rank train(): a worker outlived its time limit")
                p.kill()
    assert not _BROKEN, _BROKEN
    res = sorted(res, key=lambda r: r[0])
    for r in res:
        assert r[1] == "ok", r[2]
    assert [p.exitcode for p in procs] == [0, 0]
    seconds = time.perf_counter() - start
    print("two-rank train(): %.1f s" % seconds)
    return run, [r[2] for r in res], seconds


def test_train_on_two_ranks(two_rank_run):
    """Measured: 13 - 21 s for the pair of workers (build, two epochs, evaluation, checkpoint)."""
    run, (a, b), _ = two_rank_run
    # the loaders: rank and world from the group, the global batch of 2 as one sample per rank, two steps per epoch
    for out, rank in ((a, 0), (b, 1)):
        assert out["loaders"] == {m: {d: (rank, 2, 2, 1, 4, 2) for d in ("r", "s")} for m in ("train", "val")}
    assert a["orders"] == b["orders"] and all(sorted(o) == list(range(5)) for o in a["orders"].values())
    # one epoch by hand: parameters in lock-step, BatchNorm statistics per rank; none differs after the broadcast
    for out in (a, b):
        assert out["after_epoch"]["G.p"][0] == 0 and out["after_epoch"]["G.p"][1] > 100
        assert out["after_epoch"]["D.p"][0] == 0 and out["after_epoch"]["D.p"][1] > 10
        assert out["after_epoch"]["G.b"][0] >= 1, "the ranks read different samples: their running statistics must differ"
        assert out["after_broadcast"]["G.b"][0] == 0
        assert out["after_broadcast"]["D.b"] is None or out["after_broadcast"]["D.b"][0] == 0
    # train() for one more epoch
    for out in (a, b):
        assert out["counters"] == (4, 2, "train")
        assert len(out["results"]) == 1
        res = out["results"][0]
        assert set(res) == {"losses", "metrics"} and set(res["metrics"]) == {"r", "s"} and len(res["losses"]) >= 8
        for tab in res["metrics"].values():
            assert set(tab) == {"m", "s"} and all(set(v) == {"accuracy", "mIOU"} for v in tab.values())
    assert a["results"] == b["results"]
    assert a["last_metrics"] == b["last_metrics"]
    # one checkpoint, rank 0's, and it is the model both ranks hold
    assert [p.name for p in (run / "checkpoints").iterdir() if p.name.startswith("latest")] == ["latest_ckpt.pth"]
    for out in (a, b):
        assert out["ckpt"][:2] == (2, 4) and {"G", "D", "g_opt", "d_opt"} <= set(out["ckpt"][2])
        assert out["ckpt_G_keys"][0] == out["ckpt_G_keys"][1] > 100
        assert out["ckpt_G_differs"] == [] and out["ckpt_D_differs"] == []
    # the tables and the epoch's line are rank 0's
    assert "epoch 1: 2 steps" in a["stdout"] and "metrics_val_r" in a["stdout"] and "metrics_val_s" in a["stdout"]
    assert "epoch " not in b["stdout"] and "metrics_" not in b["stdout"]


def test_evaluation_does_not_depend_on_the_world_size(fixture, two_rank_run):
    """One process, no group, on the checkpoint the two ranks wrote: ``eval_images`` gives, table for table, what the two
    ranks computed from that state (their workers evaluated once more after ``train()`` had saved it: the tables inside
    ``train()`` belong to the state before the evaluation's own power iterations of the mask decoder's spectral norm, which
    no file holds).  Measured: 3.4 - 3.9 s."""
    from climategan_amd import parallel, train
    from climategan_amd.trainer import Trainer
    run, (a, b), _ = two_rank_run
    assert not parallel.is_distributed()
    # (the workers drove the Trainer themselves: the options the command would have written)
    (run / "opts.yaml").write_text(yaml.safe_dump(train.plain(loop_opts(fixture, run, epochs=1))))
    T = Trainer.resume_from_path(run, inference=False, device="cuda", verbose=0)
    assert T.epoch == 2 and T.global_step == 4 and T.g_reducer is None
    tables = _tables_of(T)
    close(T)
    assert len(tables) == 3 and all(set(tab) == {"m", "s"} for tab in tables)
    assert a["ckpt_tables"] == b["ckpt_tables"]
    for k, what in enumerate(("val r", "val s", "val r, one image")):
        assert tables[k] == a["ckpt_tables"][k], (what, tables[k], a["ckpt_tables"][k])
    assert tables[2] != tables[0]                       # (one image is not two)
    # rank 1 scored no image of the last call and still left with rank 0's spectral-norm vectors
    assert a["after_eval"][0] == 0 and b["after_eval"][0] == 0


# ---- 3, 4: the command -----------------------------------------------------------------------------------------------
DIST_VARIABLES = ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                  "CGAN_DDP_SINGLE_RANK_TEST")


def _config(root, tmp_path, run):
    from climategan_amd import train
    cfg = tmp_path / ("cfg_%s.yaml" % run.name)
    opts = loop_opts(root, run, epochs=1)
    cfg.write_text(yaml.safe_dump({k: train.plain(opts[k]) for k in ("tasks", "data", "comet")}))
    return cfg


def _run_children(name, tmp_path, commands_and_envs):
    """Start the commands as fresh processes, all at once, each with its own environment on top of this one's without
    the launcher's variables; wait ``CLI_TIMEOUT_S`` for all of them.  Returns ([exit status], [output], seconds)."""
    base = {k: v for k, v in os.environ.items() if k not in DIST_VARIABLES}
    start = time.perf_counter()
    procs, logs = [], []
    for k, (cmd, env) in enumerate(commands_and_envs):
        log = tmp_path / ("%s_%d.log" % (name, k))
        logs.append(log)
        with open(log, "w") as f:
            procs.append(subprocess.Popen(cmd, cwd=ROOT, env=dict(base, **env), stdout=f, stderr=subprocess.STDOUT, text=True))
    deadline = time.monotonic() + CLI_TIMEOUT_S
    try:
        for p in procs:
            try:
                p.wait(timeout=max(0.0, deadline - time.monotonic()))
            except subprocess.TimeoutExpired:
                _BROKEN.append("%s: a child ran longer than %d s" % (name, CLI_TIMEOUT_S))
                break
            if p.returncode in FATAL:
                _BROKEN.append("%s: a child ended with status %d" % (name, p.returncode))
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    outputs = [log.read_text() for log in logs]
    assert not _BROKEN, (_BROKEN, [o[-2000:] for o in outputs])
    return [p.returncode for p in procs], outputs, time.perf_counter() - start


def _command(cfg, run, *more):
    return [sys.executable, "-m", "climategan_amd.train", "--config", str(cfg), "--output", str(run), "--seed", "5", *more,
            "train.epochs=1", "train.fid.n_images=3"]


def test_the_command_on_two_ranks(fixture, tmp_path):
    """What ``torch.distributed.run`` would start, without depending on it: two children with the launcher's variables.
    Measured: 11 - 16 s."""
    _needs_healthy_children()
    run = tmp_path / "cli_run"
    cfg = _config(fixture, tmp_path, run)
    port = _free_port()
    cmd = _command(cfg, run, "--backend", "gloo", "--dist-timeout", "120")
    envs = [dict(RANK=str(r), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port)) for r in range(2)]
    codes, outputs, seconds = _run_children("two_ranks", tmp_path, [(cmd, env) for env in envs])
    print("the command on two ranks: %.1f s" % seconds)
    assert codes == [0, 0], [o[-2000:] for o in outputs]
    assert [p.name for p in run.iterdir() if p.name.startswith("opts")] == ["opts.yaml"]
    assert [p.name for p in (run / "checkpoints").iterdir()] == ["latest_ckpt.pth"]
    written = yaml.safe_load((run / "opts.yaml").read_text())
    assert written["train"]["epochs"] == 1 and written["data"]["loaders"]["batch_size"] == 2
    saved = torch.load(run / "checkpoints" / "latest_ckpt.pth", map_location="cpu", weights_only=False)
    assert saved["epoch"] == 1 and saved["step"] == 2 and {"G", "D", "g_opt", "d_opt"} <= set(saved)
    assert all(torch.isfinite(v.float()).all() for v in saved["G"].values())
    assert "epoch 0: 2 steps" in outputs[0] and "metrics_val_r" in outputs[0] and "train: 1 epochs into" in outputs[0]
    assert "epoch 0" not in outputs[1] and "metrics_" not in outputs[1] and "train: 1 epochs" not in outputs[1]


def test_the_command_on_a_one_rank_rccl_group_equals_the_plain_command(fixture, tmp_path):
    """The reducers, the loaders' seed broadcast, ``agree``, the buffer broadcast, the gathers of the evaluation and the
    barriers through RCCL with one rank (``CGAN_DDP_SINGLE_RANK_TEST=1``, as tests/test_gpu_train.py): the average over one
    rank is exact in fp32, so the checkpoint is the plain command's, bit for bit.  Measured: 8.6 - 8.9 s for the RCCL run and 5.9 s for the
    plain one; 0 of 759 / 40 / 774 / 40 tensors of G / D / g_opt / d_opt differ."""
    _needs_healthy_children()
    runs = [tmp_path / "rccl_run", tmp_path / "plain_run"]
    cfgs = [_config(fixture, tmp_path, run) for run in runs]
    env = dict(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()),
               CGAN_DDP_SINGLE_RANK_TEST="1")
    codes, outputs, seconds = _run_children("one_rank_rccl", tmp_path, [(_command(cfgs[0], runs[0], "--backend", "nccl"), env)])
    print("the command on one RCCL rank: %.1f s" % seconds)
    assert codes == [0], outputs[0][-3000:]
    assert "GradBucketReducer:" in outputs[0] and "1 ranks over nccl" in outputs[0] and "epoch 0: 2 steps" in outputs[0]
    codes, plain_outputs, seconds = _run_children("plain", tmp_path, [(_command(cfgs[1], runs[1]), {})])
    print("the plain command: %.1f s" % seconds)
    assert codes == [0], plain_outputs[0][-3000:]
    assert "GradBucketReducer:" not in plain_outputs[0] and "epoch 0: 2 steps" in plain_outputs[0]
    a, b = [torch.load(run / "checkpoints" / "latest_ckpt.pth", map_location="cpu", weights_only=False) for run in runs]
    assert (a["epoch"], a["step"]) == (b["epoch"], b["step"]) == (1, 2)
    for entry in ("G", "D", "g_opt", "d_opt"):
        ta, tb = _tensors(a[entry], entry), _tensors(b[entry], entry)
        assert list(ta) == list(tb) and len(ta) > 10
        differ = [k for k in ta if not torch.equal(ta[k], tb[k])]
        worst = max((float((ta[k].double() - tb[k].double()).abs().max()) for k in differ), default=0.0)
        print("%s: %d of %d tensors differ, largest difference %.3e" % (entry, len(differ), len(ta), worst))
        assert not differ, (entry, len(differ), len(ta), worst, differ[:5])
