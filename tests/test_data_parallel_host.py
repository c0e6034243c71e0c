"""The host side of the data-parallel train command, on CPU: the loaders' rank shards of ONE shared permutation
(``data.OmniLoader(rank=, world=)``), the small collectives of ``climategan_amd/parallel.py`` (``agree``,
``gather_in_order``) between two gloo ranks, and the command's new options.  The dataset is tests/loader_fixture.py's; the
loaders run with ``device="cpu"`` and an identity transform, which stages nothing.  Every equality is exact."""
import datetime
import os
import socket
import sys
import time
from pathlib import Path

import pytest
import torch

import loader_fixture as lf

ROOT = Path(__file__).resolve().parent.parent
GROUP_TIMEOUT_S = 60


def identity(samples):
    return samples


def loader(root, batch_size, max_samples=-1, **kw):
    from climategan_amd.data import OmniListDataset, OmniLoader
    opts = lf.fixture_opts(root)
    opts.data.max_samples = max_samples
    return OmniLoader(OmniListDataset("train", "r", opts, device="cpu"), batch_size, device="cpu", transform=identity, **kw)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    path = tmp_path_factory.mktemp("dp_host")
    lf.write(path)
    return path


# ---- 1. sharding without a group -------------------------------------------------------------------------------------
def test_rank_shards_tile_the_one_process_batches(root):
    single = loader(root, 4).seed(11)
    ranks = [loader(root, 4, rank=r, world=2).seed(11) for r in range(2)]
    assert len(single.dataset) == 5
    assert len(single) == len(ranks[0]) == len(ranks[1]) == 1
    assert [ld.batch_size for ld in ranks] == [4, 4] and [ld.local_batch_size for ld in ranks] == [2, 2]
    assert (single.batch_size, single.local_batch_size, single.rank, single.world) == (4, 4, 0, 1)
    for _epoch in range(3):                                     # a fresh permutation per epoch, still shared
        whole, parts = single.batches(), [ld.batches() for ld in ranks]
        assert len(whole) == len(parts[0]) == len(parts[1]) == 1
        for k in range(len(whole)):
            assert len(parts[0][k]) == len(parts[1][k]) == 2
            assert parts[0][k] + parts[1][k] == whole[k]
        assert ranks[0].last_order == ranks[1].last_order == single.last_order
    # more than one step per epoch, and the collated batch holds the rank's samples alone
    single2 = loader(root, 2).seed(11)
    ranks2 = [loader(root, 2, rank=r, world=2).seed(11) for r in range(2)]
    whole, parts = single2.batches(), [ld.batches() for ld in ranks2]
    assert len(whole) == 2 and all(parts[0][k] + parts[1][k] == whole[k] for k in range(2))
    ranks2[1].seed(11)
    items = list(ranks2[1])
    assert len(items) == 2 and all(item["domain"] == ["r"] and len(item["paths"]["x"]) == 1 for item in items)
    assert [item["paths"]["x"][0] for item in items] == [ranks2[1].dataset.samples_paths[p[0]]["x"] for p in parts[1]]


def test_a_batch_the_world_does_not_divide_is_refused(root):
    with pytest.raises(ValueError, match="cannot be split evenly"):
        loader(root, 3, rank=0, world=2)
    with pytest.raises(ValueError, match="cannot be split evenly"):
        loader(root, 1, rank=1, world=2)
    with pytest.raises(ValueError, match="outside a world"):
        loader(root, 4, rank=2, world=2)


def test_world_of_one_is_the_loader_as_it_was(root):
    """rank 0 of 1, given or not: the lists are the permutation cut into ``batch_size`` pieces, seeded from torch's default
    generator when ``seed`` is not called, exactly as before there were ranks"""
    for kw in ({}, {"rank": 0, "world": 1}):
        ld = loader(root, 2, **kw).seed(11)
        lists = ld.batches()
        order = torch.randperm(5, generator=torch.Generator().manual_seed(11)).tolist()
        assert ld.last_order == order and lists == [order[0:2], order[2:4]]
        torch.manual_seed(3)
        a = loader(root, 2, **kw).batches()
        torch.manual_seed(3)
        expected_seed = int(torch.empty((), dtype=torch.int64).random_().item())
        order = torch.randperm(5, generator=torch.Generator().manual_seed(expected_seed)).tolist()
        assert a == [order[0:2], order[2:4]]
        assert loader(root, 2, shuffle=False, **kw).batches() == [[0, 1], [2, 3]]


def test_reader_threads_share_the_machines_cpus(root, monkeypatch):
    assert loader(root, 2, num_workers=64).num_workers == 16                # no variable: as before
    for local_world, asked, want in ((8, 6, 2), (2, 6, 6), (2, 12, 8), (32, 6, 1), (8, 0, 0), (1, 64, 16)):
        monkeypatch.setenv("LOCAL_WORLD_SIZE", str(local_world))
        assert loader(root, 2, num_workers=asked).num_workers == want == min(asked, 16, max(1, 16 // local_world))


def test_get_loader_passes_rank_and_world_through(root, monkeypatch):
    from climategan_amd import data
    monkeypatch.setattr(data, "compile_transforms", lambda *a, **k: identity)
    opts = lf.fixture_opts(root)
    opts.data.loaders.batch_size = 4
    ld = data.get_loader("train", "r", opts, device="cpu", rank=1, world=2)
    assert (ld.batch_size, ld.local_batch_size, ld.rank, ld.world) == (4, 2, 1, 2)
    loaders = data.get_all_loaders(opts, 1, "cpu", rank=1, world=4)
    assert all(v.local_batch_size == 1 and v.rank == 1 for d in loaders.values() for v in d.values())
    assert data.get_loader("train", "r", opts, 1, "cpu").local_batch_size == 4          # the present signatures
    opts.train.kitti.pretrain = True                                                       # kitti's own batch size: 1
    with pytest.raises(ValueError, match="cannot be split evenly"):
        data.get_loader("train", "kitti", opts, device="cpu", rank=0, world=2)


# ---- 2-4. two gloo ranks ---------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, root, q):
    try:
        sys.path.insert(0, str(ROOT))
        sys.path.insert(0, str(ROOT / "tests"))
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        import torch.distributed as dist
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=GROUP_TIMEOUT_S))
        from climategan_amd import parallel
        out = {"rank": (parallel.rank(), parallel.world(), parallel.is_main(), parallel.is_distributed())}

        # 2. loaders from the group: one permutation although the ranks' generators differ
        torch.manual_seed(100 + rank)
        ld = loader(root, 4)
        out["loader"] = (ld.rank, ld.world, ld.local_batch_size, [ld.batches() for _ in range(3)], ld.last_order)
        ld.seed(11)
        out["seeded"] = ld.batches()

        # 3. agree
        start = time.perf_counter()
        same = {("train", "r"): (5, 4), ("val", "r"): (5, 4)}
        out["agree_ok"] = parallel.agree("the loaders", dict(same)) == same and parallel.agree("opts.tasks", ["d", "s", "m"])
        short = loader(root, 4, max_samples=3 if rank == 1 else -1)        # rank 1 lists fewer files
        try:
            parallel.agree("the loaders' (len(dataset), batch_size)",
                           {("train", "r"): (len(short.dataset), short.batch_size), ("val", "r"): (5, 4)})
            out["agree_bad"] = None
        except ValueError as e:
            out["agree_bad"] = str(e)
        try:
            parallel.agree("opts.tasks", ["d", "s", "m"] if rank == 0 else ["d", "s"])
            out["agree_tasks"] = None
        except ValueError as e:
            out["agree_tasks"] = str(e)
        out["agree_seconds"] = time.perf_counter() - start

        # 4. gather_in_order
        values = {0: 0.125, 1: 1.0 / 3.0, 2: 2.5, 3: 1e-9, 4: 7.0}
        mine = [(i, values[i]) for i in ((0, 2, 4) if rank == 0 else (1, 3))]
        out["gather"] = parallel.gather_in_order(reversed(mine))
        out["gather_one_empty"] = parallel.gather_in_order(mine if rank == 0 else [])
        out["gather_all_empty"] = parallel.gather_in_order([])
        out["mean"] = parallel.mean_over_ranks({"G.a": 0.1 + rank, "G.b": 3.0})

        # broadcast_buffers: rank 0's running statistics, parameters untouched
        bn = torch.nn.BatchNorm1d(3)
        with torch.no_grad():
            bn.running_mean.fill_(1.0 + rank)
            bn.weight.fill_(5.0 + rank)
        version = bn.running_mean._version
        parallel.broadcast_buffers(bn)
        out["buffers"] = (bn.running_mean.tolist(), bn.weight.tolist(), bn.running_mean._version > version)
        q.put((rank, "ok", out))
        parallel.barrier()
        parallel.shutdown()
        assert not dist.is_initialized()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))


@pytest.fixture(scope="module")
def two_ranks(root):
    """One pair of gloo ranks runs every collective case of this file once; the tests below read what they returned."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, root, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
        for p in procs:
            p.join(timeout=60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    for r in res:
        assert r[1] == "ok", r[2]
    assert [p.exitcode for p in procs] == [0, 0]
    return [r[2] for r in res]


def test_loaders_in_a_group_share_rank_zeros_permutation(two_ranks):
    a, b = two_ranks
    assert a["rank"] == (0, 2, True, True) and b["rank"] == (1, 2, False, True)
    assert a["loader"][:3] == (0, 2, 2) and b["loader"][:3] == (1, 2, 2)           # rank and world from the group
    assert a["loader"][4] == b["loader"][4] and sorted(a["loader"][4]) == list(range(5))
    for ea, eb in zip(a["loader"][3], b["loader"][3]):                              # three epochs, one step each
        assert len(ea) == len(eb) == 1 and len(ea[0]) == len(eb[0]) == 2
        assert not set(ea[0]) & set(eb[0])
    last = a["loader"][4]
    assert a["loader"][3][2][0] + b["loader"][3][2][0] == last[:4]                  # complementary: the global batch
    order = torch.randperm(5, generator=torch.Generator().manual_seed(11)).tolist()
    assert a["seeded"] == [order[0:2]] and b["seeded"] == [order[2:4]]              # seed(n) keeps working


def test_agree_passes_equal_values_and_names_the_entry_that_differs(two_ranks):
    for out in two_ranks:
        assert out["agree_ok"] == ["d", "s", "m"]
        msg = out["agree_bad"]
        assert msg is not None, "ranks with different dataset lengths were not stopped"
        assert "('train', 'r')" in msg and "(5, 4)" in msg and "(3, 4)" in msg and "rank 1" in msg
        assert "len(dataset)" in msg and "('val', 'r')" not in msg
        assert out["agree_tasks"] is not None and "opts.tasks" in out["agree_tasks"]
        assert out["agree_seconds"] < GROUP_TIMEOUT_S
    assert two_ranks[0]["agree_bad"] == two_ranks[1]["agree_bad"]


def test_gather_in_order_gives_every_rank_the_values_by_index(two_ranks):
    for out in two_ranks:
        assert out["gather"] == [0.125, 1.0 / 3.0, 2.5, 1e-9, 7.0]
        assert out["gather_one_empty"] == [0.125, 2.5, 7.0]
        assert out["gather_all_empty"] == []
        assert out["mean"] == {"G.a": (0.1 + 1.1) / 2, "G.b": 3.0}
        assert out["buffers"] == ([1.0, 1.0, 1.0], [5.0 + two_ranks.index(out)] * 3, True)


def test_helpers_without_a_group():
    from climategan_amd import parallel
    assert (parallel.rank(), parallel.world(), parallel.is_main(), parallel.is_distributed()) == (0, 1, True, False)
    parallel.barrier()
    parallel.shutdown()
    assert parallel.gather_in_order([(3, "c"), (1, "a")]) == ["a", "c"]
    assert parallel.agree("x", {"k": 1}) == {"k": 1}
    assert parallel.mean_over_ranks({"G.a": 0.25}) == {"G.a": 0.25}
    bn = torch.nn.BatchNorm1d(2)
    version = bn.running_mean._version
    parallel.broadcast_buffers(bn)
    assert bn.running_mean._version == version


# ---- 5. the command's options ----------------------------------------------------------------------------------------
def test_cli_options_and_init_from_env(monkeypatch):
    import torch.distributed as dist

    from climategan_amd import parallel, train
    args = train.parse_args(["--backend", "gloo", "--dist-timeout", "120", "--seed", "5", "train.epochs=1"])
    assert (args.backend, args.dist_timeout, args.seed, args.overrides) == ("gloo", 120.0, 5, ["train.epochs=1"])
    args = train.parse_args([])
    assert (args.backend, args.dist_timeout, args.seed) == ("nccl", None, None)
    with pytest.raises(SystemExit):
        train.parse_args(["--backend", "mpi"])
    with pytest.raises(SystemExit):
        train.parse_args(["--seed", "x"])
    for name in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(name, raising=False)
    assert parallel.init_from_env() == (0, 1) and parallel.init_from_env("gloo", 5) == (0, 1)
    assert not dist.is_initialized()
    assert "torch.distributed.run --nproc-per-node 8" in train.__doc__ and "-m climategan_amd.train" in train.__doc__


def test_seed_everything_seeds_the_three_generators():
    import random

    import numpy as np

    from climategan_amd import train
    train.seed_everything(5)
    a = (random.random(), float(np.random.rand()), float(torch.rand(())))
    train.seed_everything(5)
    assert (random.random(), float(np.random.rand()), float(torch.rand(()))) == a
    train.seed_everything(6)
    assert (random.random(), float(np.random.rand()), float(torch.rand(()))) != a
