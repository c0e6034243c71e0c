"""The cases of tests/golden/data_decode.npz, shared by the script that writes the fixture from the real reference
(tests/devtools/make_golden_data_decode.py) and the tests that read it (test_data_decode_host.py, test_gpu_data_decode.py).
The raw sources come from ``climategan_amd.fill``, so the fixture holds the reference's outputs only."""
import numpy as np

import data_transform_cases as dc
from climategan_amd import fill

H, W = 64, 96           # small: the reference's encode_segmap is a Python loop over every pixel
FAR = 1000
BOUNDS = dict(min=0.35, max=6.95, buckets=256)       # defaults.yaml:129-134, as data_transform_cases.case_opts


def _u(name, shape):
    return fill.uniform01(shape, fill.key_seed("decode." + name, 5))


def _bytes(name, shape, lo=0, hi=256):
    return (lo + np.floor(_u(name, shape) * (hi - lo))).astype(np.uint8)


def unity(name, h=H, w=W, channels=3):
    """Unity depth code with R, G in 0..247 (the 31 slices the simulator writes) and no code 0"""
    rgb = np.concatenate([_bytes(name + ".rg", (h, w, 2), 0, 248), _bytes(name + ".b", (h, w, 1))], axis=2)
    zero = (rgb[..., 0] == 247) & (rgb[..., 1] == 247) & (rgb[..., 2] == 255)
    rgb[zero, 2] = 254
    if channels == 4:
        rgb = np.concatenate([rgb, np.full((h, w, 1), 255, np.uint8)], axis=2)
    return rgb


def unity_quirks(name):
    """R / G in 248..255 (a truncated division: 248..254 -> 0, 255 -> -1, so a negative code) and the code 0"""
    rgb = unity(name)
    sel = _u(name + ".sel", (H, W))
    hi = _bytes(name + ".hi", (H, W, 2), 248, 256)
    rgb[sel < 0.15, 0] = hi[sel < 0.15, 0]
    rgb[(sel > 0.1) & (sel < 0.3), 1] = hi[(sel > 0.1) & (sel < 0.3), 1]
    rgb[sel > 0.97] = (247, 247, 255)
    rgb[0, 0] = (255, 255, 255)
    rgb[0, 1] = (255, 0, 0)
    rgb[0, 2] = (250, 254, 255)         # code 0 through the truncation
    return rgb


def kitti_depth(name, h=H, w=W):
    """uint16 centimetres over the whole range, never 0"""
    v = (1 + np.floor(_u(name, (h, w)) * 65535)).astype(np.uint16)
    v[0, :4] = (1, 65535, 100, 99)
    return v


def real_depth(name, nan=False):
    v = fill.uniform((H, W), fill.key_seed("decode." + name, 5), 0.25, 80.0).astype(np.float32)
    if nan:
        v[H // 2, W // 3] = np.nan
    return v


def mask(name, top, channels=0, h=H, w=W):
    m = ((_u(name, (h, w)) > 0.5) * top).astype(np.uint8)
    if channels:
        rest = _bytes(name + ".rest", (h, w, channels - 1), 0, 256 if top > 127 else 2)
        m = np.concatenate([m[..., None], rest], axis=2)
    return m


def kitti_seg(name, classes, h=H, w=W):
    """every kitti colour, plus off-palette pixels (random bytes, and colours one step off)"""
    cols = np.array(list(classes.values()), np.uint8)
    idx = np.floor(_u(name, (h, w)) * (len(cols) + 3)).astype(np.int64)
    out = _bytes(name + ".off", (h, w, 3))
    on = idx < len(cols)
    out[on] = cols[idx[on]]
    near = idx == len(cols)
    out[near] = cols[np.floor(_u(name + ".n", (h, w)) * len(cols)).astype(np.int64)][near] ^ 1
    out[0, :len(cols)] = cols
    return out


def ties(classes, count=48):
    """RGBA pixels whose two nearest palette colours lie at the same squared distance (searched on a lattice)"""
    cols = np.array(list(classes.values()), np.int64)
    r, g, b = np.meshgrid(np.arange(256), np.arange(256), np.unique(np.concatenate([cols[:, 2], [128, 30, 158]])), indexing="ij")
    px = np.stack([r.ravel(), g.ravel(), b.ravel(), np.full(r.size, 255)], axis=1)
    d = ((px[:, None, :] - cols[None]) ** 2).sum(-1)
    two = np.sort(d, axis=1)[:, :2]
    hit = px[two[:, 0] == two[:, 1]]
    assert len(hit) >= 8, len(hit)
    return hit[np.linspace(0, len(hit) - 1, min(count, len(hit))).astype(np.int64)].astype(np.uint8)


def palette_seg(name, classes, h=H, w=W):
    """exact colours, perturbed colours (any alpha) and constructed ties"""
    cols = np.array(list(classes.values()), np.int64)
    idx = np.floor(_u(name, (h, w)) * len(cols)).astype(np.int64)
    out = cols[idx]
    noise = np.floor(_u(name + ".noise", (h, w, 4)) * 121).astype(np.int64) - 60
    noisy = _u(name + ".sel", (h, w)) > 0.5
    out[noisy] = np.clip(out[noisy] + noise[noisy], 0, 255)
    out = out.astype(np.uint8)
    t = ties(classes)
    out[1, :len(t)] = t
    far_off = _u(name + ".far", (h, w)) > 0.93
    out[far_off] = _bytes(name + ".rand", (h, w, 4))[far_off]
    return out


def x_image(name, h=H, w=W, channels=3):
    return _bytes(name, (h, w, channels), 20, 221)          # min > 0 and max < 255: the normalisation does something


# name -> (task, domain, source builder, tensor_loader options)
def single_cases(classes_dict):
    o = lambda normalize=False, log=False: dict(normalize=normalize, log=log)   # noqa: E731
    return {
        "unity_inv": ("d", "s", lambda: unity("unity_inv"), o()),
        "unity_log": ("d", "s", lambda: unity("unity_log"), o(log=True)),
        "unity_norm": ("d", "s", lambda: unity("unity_norm"), o(normalize=True)),
        "unity_rgba": ("d", "s", lambda: unity("unity_rgba", channels=4), o(normalize=True)),
        "unity_quirks_inv": ("d", "s", lambda: unity_quirks("unity_quirks"), o()),
        "unity_quirks_log": ("d", "s", lambda: unity_quirks("unity_quirks"), o(log=True)),
        "kitti_inv": ("d", "kitti", lambda: kitti_depth("kitti_inv"), o()),
        "kitti_log": ("d", "kitti", lambda: kitti_depth("kitti_log"), o(log=True)),
        "kitti_norm": ("d", "kitti", lambda: kitti_depth("kitti_norm"), o(normalize=True)),
        "real": ("d", "r", lambda: real_depth("real"), o()),
        "real_nan": ("d", "r", lambda: real_depth("real_nan", nan=True), o()),
        "mask_255": ("m", "r", lambda: mask("mask_255", 255), o()),
        "mask_01": ("m", "r", lambda: mask("mask_01", 1), o()),
        "mask_3c": ("m", "r", lambda: mask("mask_3c", 255, channels=3), o()),
        "kitti_seg": ("s", "kitti", lambda: kitti_seg("kitti_seg", classes_dict["kitti"]), o()),
        "palette_s": ("s", "s", lambda: palette_seg("palette_s", classes_dict["s"]), o()),
        "palette_r": ("s", "r", lambda: palette_seg("palette_r", classes_dict["r"]), o()),
        "x_raw": ("x", "r", lambda: x_image("x_raw"), o()),
    }


LOG_CASES = ("unity_log", "unity_quirks_log", "kitti_log")

# raw sources through the default train pipeline at small sizes, bucketized log depth included
E2E = {
    "e2e_sim": dict(items=dc.SMALL, mode="train", domain="s", seed=21, classify=True, samples=[(96, 144), (130, 90)]),
    "e2e_kitti": dict(items=dc.SMALL, mode="train", domain="kitti", seed=22, classify=True, samples=[(90, 130), (96, 144)]),
}
E2E_TASKS = ("x", "m", "d", "s")


def boundaries():
    import torch
    return torch.linspace(BOUNDS["min"], BOUNDS["max"], BOUNDS["buckets"] - 1).numpy()


def log_depth64(domain, raw):
    """float64 log of the fp32 depth of a raw depth source (the kernel's formula, restated)"""
    if domain == "s":
        r, g, b = (raw[..., k].astype(np.int32) for k in range(3))
        code = ((247 - r) / 8).astype(np.int32) * (256 * 31) + ((247 - g) / 8).astype(np.int32) * 256 + (255 - b)
        depth = code.astype(np.float32) / np.float32(246015) * np.float32(FAR)
    else:
        depth = raw.astype(np.float32) / np.float32(100)
    with np.errstate(all="ignore"):
        return np.log(depth.astype(np.float64))


def ulps_from_boundaries(domain, raw):
    """distance of every pixel's log depth to the nearest bucket boundary, in fp32 ulps of the value"""
    lg = log_depth64(domain, raw)
    gap = np.abs(lg[..., None] - boundaries().astype(np.float64)).min(-1)
    return gap / np.spacing(np.abs(lg).astype(np.float32)).astype(np.float64)


def e2e_sources(name, k, hw, classes_dict):
    """{task: raw numpy source} of sample ``k`` of the end-to-end case ``name``; the depth keeps 4 ulp from every boundary"""
    domain, (h, w) = E2E[name]["domain"], hw
    tag = "%s.%d" % (name, k)
    if domain == "s":
        d = unity(tag + ".d", h, w)
        s = palette_seg(tag + ".s", classes_dict["s"], h, w)
    else:
        d = kitti_depth(tag + ".d", h, w)
        s = kitti_seg(tag + ".s", classes_dict["kitti"], h, w)
    for _ in range(4):
        close = ulps_from_boundaries(domain, d) < 4
        if not close.any():
            break
        if domain == "s":
            d[close, 2] ^= 1
        else:
            d[close] += 1
    return {"x": x_image(tag + ".x", h, w), "m": mask(tag + ".m", 255, h=h, w=w), "d": d, "s": s}


def e2e_opts(case):
    """what ``tensor_loader`` and ``get_transforms`` read, as plain data"""
    opts = dc.case_opts(case)
    opts["train"] = {"pseudo": {"tasks": []}}
    return opts


def loader_opts(normalize, log):
    return {"train": {"pseudo": {"tasks": ["d"] if normalize else []}}, "gen": {"d": {"classify": {"enable": bool(log)}}}}
