"""The host side of the loaders (climategan_amd/data.py: OmniListDataset, OmniLoader), ``utils.get_display_indices`` and the
option handling of ``python -m climategan_amd.train``: everything that needs no GPU.  The dataset is written into
``tmp_path`` by tests/loader_fixture.py; the loader runs with ``device="cpu"`` and a stub transform, which stages nothing."""
import json

import numpy as np
import pytest
import torch

import loader_fixture as lf
from climategan_amd.config import Opts
from helpers import GOLDEN


@pytest.fixture(scope="module")
def fixture(tmp_path_factory):
    root = tmp_path_factory.mktemp("loaders")
    return root, lf.write(root)


def dataset(root, mode, domain, tasks=("d", "s", "m"), **data_opts):
    from climategan_amd.data import OmniListDataset
    opts = lf.fixture_opts(root, tasks)
    for k, v in data_opts.items():
        opts.data[k] = v
    return OmniListDataset(mode, domain, opts, device="cpu")


def stub(samples):
    """what the loader hands its transform: a list of {task: host array}; the 'batch' is each array's first byte"""
    return {task: torch.tensor([int(np.asarray(s[task]).reshape(-1).view(np.uint8)[0]) for s in samples]) for task in samples[0]}


def loader(root, mode="train", domain="r", tasks=("d", "s", "m"), **kw):
    from climategan_amd.data import OmniLoader
    return OmniLoader(dataset(root, mode, domain, tasks), lf.BATCH, device="cpu", transform=stub, **kw)


def test_file_lists_json_yaml_and_base_path(fixture):
    root, listed = fixture
    r = dataset(root, "train", "r")                         # "train_r.json": no "/" -> looked up in data.files.base
    assert r.file_list_path == str(root / "lists" / "train_r.json") and len(r) == 5
    assert r.samples_paths == listed["train"]["r"]
    s = dataset(root, "train", "s")                         # a YAML list
    assert s.file_list_path.endswith("train_s.yaml") and s.samples_paths == listed["train"]["s"]
    v = dataset(root, "val", "kitti")                       # a path with "/" is taken as it is
    assert v.file_list_path == str(root / "lists" / "val_kitti.json") and len(v) == 5
    opts = lf.fixture_opts(root)
    opts.data.files.train.r = str(root / "lists" / "train_r.txt")
    (root / "lists" / "train_r.txt").write_text("[]")
    from climategan_amd.data import OmniListDataset
    with pytest.raises(ValueError, match="Unknown file list type"):
        OmniListDataset("train", "r", opts, device="cpu")


def test_max_samples_and_filter_samples(fixture):
    root, _ = fixture
    assert len(dataset(root, "train", "r", max_samples=3)) == 3
    assert len(dataset(root, "train", "r", max_samples=-1)) == 5
    masker = dataset(root, "train", "s", tasks=("m", "s", "d"))
    assert masker.tasks == {"m", "s", "d", "x"} and all(set(p) == {"x", "m", "s", "d"} for p in masker.samples_paths)
    painter = dataset(root, "train", "s", tasks=("p",))     # the Painter reads x and m, whatever else the list holds
    assert painter.tasks == {"p", "x", "m"} and all(set(p) == {"x", "m"} for p in painter.samples_paths)
    no_mask = dataset(root, "train", "s", tasks=("d",))
    assert all(set(p) == {"x", "d"} for p in no_mask.samples_paths)


def test_check_samples_fails_on_a_missing_file(fixture, tmp_path):
    root, listed = fixture
    assert len(dataset(root, "val", "r", check_samples=True)) == 5
    broken = [dict(s) for s in listed["val"]["r"]]
    broken[3]["d"] = str(tmp_path / "nowhere.npy")
    path = tmp_path / "broken.json"
    path.write_text(json.dumps(broken))
    opts = lf.fixture_opts(root)
    opts.data.files.val.r = str(path)
    opts.data.check_samples = True
    from climategan_amd.data import OmniListDataset
    with pytest.raises(AssertionError, match="nowhere.npy does not exist"):
        OmniListDataset("val", "r", opts, device="cpu")


def test_env_to_path_and_the_listed_variable(fixture, monkeypatch):
    from climategan_amd.utils import env_to_path
    root, listed = fixture
    monkeypatch.setenv(lf.ENV, str(root / "train" / "rf"))
    entry = listed["train"]["rf"][0]["x"]
    assert entry.startswith("$" + lf.ENV + "/")
    assert env_to_path(entry) == str(root / "train" / "rf" / "x0.png")
    assert env_to_path("/a/b.png") == "/a/b.png"
    rf = dataset(root, "train", "rf", tasks=("p",))
    arr, known = rf.read_host(0)["x"]                       # the dataset expands the variable when it reads
    assert arr.shape == (24, 40, 3) and known["minmax"] == (arr.min(), arr.max())
    monkeypatch.delenv(lf.ENV)
    with pytest.raises(KeyError):
        rf.read_host(0)


def test_read_host_kinds(fixture):
    """the arrays as the decoders leave them: RGBA x and m lose the fourth channel, the 16-bit PNG stays uint16, the
    real depth is fp32, and the pass over the array tells min / max or the mask's threshold"""
    root, _ = fixture
    r, s, kitti = dataset(root, "train", "r"), dataset(root, "train", "s"), dataset(root, "train", "kitti")
    rgba = r.read_host(1)
    assert rgba["x"][0].shape == (40, 24, 3) and rgba["x"][0].flags["C_CONTIGUOUS"]
    assert rgba["d"][0].dtype == np.float32 and set(rgba["d"][1]) == {"minmax"}
    assert rgba["s"][0].shape == (40, 24, 4) and rgba["s"][0].dtype == np.uint8 and rgba["s"][1] == {}      # .npy
    assert r.read_host(0)["s"][0].shape == (24, 40, 4)                                                      # RGBA PNG
    assert rgba["m"][0].shape == (40, 24) and rgba["m"][1] == {"threshold": True}
    assert s.read_host(0)["d"][0].shape == (24, 40, 3) and s.read_host(0)["d"][1] == {}
    for k in (0, 1):                                        # 16-bit PNG and .npy
        d = kitti.read_host(k)["d"][0]
        assert d.dtype == np.uint16 and d.shape == lf.SIZES[k] and int(d.max()) > 255
    assert kitti.read_host(0)["s"][0].shape == (24, 40, 3)


def test_len_drops_the_last_partial_batch(fixture):
    root, _ = fixture
    ld = loader(root)
    assert len(ld.dataset) == 5 and ld.batch_size == 2 and len(ld) == 2
    assert len(list(ld)) == 2
    from climategan_amd.data import OmniLoader
    assert len(OmniLoader(ld.dataset, 5, device="cpu", transform=stub)) == 1
    assert len(OmniLoader(ld.dataset, 6, device="cpu", transform=stub)) == 0
    assert OmniLoader(ld.dataset, 2, num_workers=64, device="cpu", transform=stub).num_workers == 16


def test_permutation_is_seeded_fresh_and_without_repeats(fixture):
    root, _ = fixture
    a, b = loader(root).seed(7), loader(root).seed(7)
    epochs_a = [[i for batch in a.batches() for i in batch] for _ in range(3)]
    epochs_b = [[i for batch in b.batches() for i in batch] for _ in range(3)]
    assert epochs_a == epochs_b                             # the same seed, the same epochs
    assert len({tuple(e) for e in epochs_a}) > 1            # a fresh permutation per epoch
    for e in epochs_a:
        assert len(e) == 4 and len(set(e)) == 4 and all(0 <= i < 5 for i in e)
    assert [i for batch in loader(root).seed(8).batches() for i in batch] != epochs_a[0] or \
        [i for batch in loader(root).seed(9).batches() for i in batch] != epochs_a[0]
    # without seed(): the loader's generator is seeded from torch's default one
    torch.manual_seed(3)
    c = loader(root).batches()
    torch.manual_seed(3)
    assert loader(root).batches() == c
    plain = loader(root, shuffle=False)
    assert plain.batches() == [[0, 1], [2, 3]]


def test_collated_item(fixture):
    root, listed = fixture
    for domain in ("r", "kitti"):
        ld = loader(root, domain=domain, num_workers=2).seed(1)
        items = list(ld)
        order = ld.last_order
        assert len(items) == 2
        for k, item in enumerate(items):
            idx = order[2 * k:2 * k + 2]
            assert set(item) == {"data", "paths", "domain", "mode"}
            assert set(item["data"]) == set(item["paths"]) == {"x", "d", "s", "m"}
            assert all(v.shape == (2,) for v in item["data"].values())
            for task in item["paths"]:
                assert item["paths"][task] == [listed["train"][domain][i][task] for i in idx]
            assert item["domain"] == ["s" if domain == "kitti" else domain] * 2 and item["mode"] == ["train"] * 2
            # the stub's value is the first byte of each sample's own file
            first = [int(ld.dataset.read_host(i)["x"][0].reshape(-1)[0]) for i in idx]
            assert item["data"]["x"].tolist() == first


def test_get_all_loaders_and_batch_size_rules(fixture, monkeypatch):
    from climategan_amd import data
    root, _ = fixture
    monkeypatch.setattr(data, "_device", lambda device=None: torch.device("cpu"))
    monkeypatch.setattr(data, "compile_transforms", lambda *a, **k: stub)
    opts = lf.fixture_opts(root, tasks=("d", "s", "m", "p"))
    loaders = data.get_all_loaders(opts, device="cpu")
    assert list(loaders) == ["train", "val"] and all(list(v) == ["r", "s", "rf", "kitti"] for v in loaders.values())
    assert all(ld.batch_size == 2 and ld.num_workers == 4 for v in loaders.values() for ld in v.values())
    masker = data.get_all_loaders(lf.fixture_opts(root, tasks=("d", "s", "m")), device="cpu")
    assert list(masker["train"]) == ["r", "s", "kitti"]                 # no Painter, no rf
    del opts.data.files["val"]
    assert data.get_all_loaders(opts, device="cpu")["val"] == {}
    opts.train.kitti.pretrain = True                                    # data.py:507-514
    assert data.get_loader("train", "kitti", opts, device="cpu").batch_size == 1
    assert data.get_loader("train", "r", opts, device="cpu").batch_size == 2


def test_display_indices_equal_the_reference():
    from climategan_amd.utils import get_display_indices
    cases = json.loads((GOLDEN / "display_indices.json").read_text())
    assert len(cases) >= 8
    for case in cases:
        opts = Opts({"comet": {"display_size": case["display_size"]}, "train": {"fid": {"n_images": case["n_images"]}}})
        np.random.seed(11)
        state = np.random.get_state()[1].copy()
        got = get_display_indices(opts, case["domain"], case["length"])
        assert [int(i) for i in got] == case["indices"], case
        assert np.array_equal(state, np.random.get_state()[1])          # the global numpy generator is left alone
    assert get_display_indices(Opts({"comet": {"display_size": [4, 1]}}), "r", 9) == [4, 1]


def test_shuffle_batch_tuple_only_permutes():
    from climategan_amd.tutils import shuffle_batch_tuple
    np.random.seed(2)
    seen = set()
    for _ in range(20):
        out = shuffle_batch_tuple(("a", "b", "c"))
        assert sorted(out) == ["a", "b", "c"]
        seen.add(tuple(out))
    assert len(seen) > 1


# ---- python -m climategan_amd.train: options -------------------------------------------------------------------------
def test_cli_option_merging(tmp_path):
    from climategan_amd import train
    base = train.train_defaults()
    assert base.data.loaders.batch_size == 6 and base.train.epochs == 300 and base.train.pseudo.tasks == []
    assert base.train.kitti.pretrain is False and base.comet.display_size == 20
    assert [i.name for i in base.data.transforms] == ["hflip", "resize", "crop", "brightness", "saturation", "contrast", "resize"]
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("tasks: [d, s, m]\ntrain:\n  epochs: 7\ndata:\n  loaders:\n    batch_size: 3\n  files:\n    base: /lists\n")
    opts = train.build_opts(cfg, ["train.epochs=2", "data.files.train.r=r.json", "gen.m.use_spade=true", "output_path=/x/run",
                                  "data.loaders.num_workers=0", "comet.display_size=4", "load_paths.m=none"])
    assert opts.tasks == ["d", "s", "m"] and opts.train.epochs == 2                # file over defaults, override over file
    assert opts.data.loaders == {"batch_size": 3, "num_workers": 0}
    assert opts.data.files == {"base": "/lists", "train": {"r": "r.json"}}
    assert opts.gen.m.use_spade is True and opts.gen.m.use_advent is True          # yaml values; siblings kept
    assert opts.comet.display_size == 4 and opts.load_paths.m == "none" and opts.output_path == "/x/run"
    assert opts.train.lambdas.G.m.bce == 1                                          # untouched defaults survive
    assert train.parse_override("tasks=[p]") == (["tasks"], ["p"])
    assert train.parse_override("a.b=1e-3")[1] == "1e-3" or train.parse_override("a.b=1e-3")[1] == 1e-3
    assert train.parse_override("a.b=0.001") == (["a", "b"], 0.001)
    args = train.parse_args(["--config", str(cfg), "--output", "/o", "--dtype", "fp16", "train.epochs=1"])
    assert (args.config, args.output, args.dtype, args.overrides, args.resume) == (str(cfg), "/o", "fp16", ["train.epochs=1"], None)
    dumped = train.plain(opts)
    assert type(dumped) is dict and type(dumped["data"]["transforms"][0]) is dict


def test_cli_refusals(tmp_path):
    from climategan_amd import train
    for arg, word in [("comet.rows_per_log=5", "comet"), ("comet.exp_id=abc", "comet"), ("jobs=[a]", "SLURM"),
                      ("hydra.run.dir=/x", "hydra"), ("+experiment=foo", "hydra"), ("train.auto_resume=true", "--resume")]:
        with pytest.raises(SystemExit, match=arg.split("=")[0].lstrip("+")) as e:
            train.parse_args([arg])
        assert word in str(e.value)
    with pytest.raises(SystemExit, match="key.sub=value"):
        train.parse_args(["train.epochs"])
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("comet:\n  display_size: 3\n  rows_per_log: 5\n")
    with pytest.raises(SystemExit, match="comet.rows_per_log"):
        train.build_opts(cfg)
    cfg.write_text("comet:\n  display_size: 3\n")
    assert train.build_opts(cfg).comet.display_size == 3
    with pytest.raises(SystemExit):
        train.parse_args(["--dtype", "fp32"])
    with pytest.raises(SystemExit, match="no file lists"):
        train.main(["train.epochs=1"])
