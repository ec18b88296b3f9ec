"""What the test files share: the golden loaders, the trained fixture net and its grids, the helpers of the
training-march tests (batches, losses, flat gradients, the grid file, the trainer), the long-segment case of the
distortion and background tests, the cfg-restoring helpers and a few one-liners of the CPU and data-parallel tests.

A plain module: a test file imports the helpers and fixtures it uses by name (an imported fixture is cached
per importing module, as when each file defined its own).  The fp64 references the kernels are checked against
are NOT here: each stays in the file whose kernels it checks.
"""
import contextlib
import os
import re
import socket

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MAPS = ("rgb_map_f", "depth_map_f", "acc_map_f")


# --------------------------------------------------------------------------------------
# modules and the library as fixtures
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def O():
    from oracle import nerf_oracle
    return nerf_oracle


@pytest.fixture(scope="module")
def ops():
    from nerf_amd import ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from nerf_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _lib.lib()


@pytest.fixture(scope="module")
def built_lib():
    """``lib`` for the files that do not skip (imported ``as lib``)."""
    from nerf_amd import _lib
    return _lib.lib()  # (raises when the library is not built)


def _declared(text, name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# --------------------------------------------------------------------------------------
# cfg.task_arg, restored after a test
# --------------------------------------------------------------------------------------
@contextlib.contextmanager
def restored_keys(ta, keys):
    """``ta`` itself; on exit its ``keys`` are what they were (one that was absent is removed)."""
    old = {k: ta[k] for k in keys if k in ta}
    yield ta
    for k in keys:
        if k in old:
            ta[k] = old[k]
        else:
            ta.pop(k, None)


def fp32_cfg(keys):
    """The body of a GPU test file's ``*_cfg`` fixture (``yield from``): cfg at perturb 0 and mlp_dtype fp32,
    with the file's ``keys`` of task_arg (these two among them) restored afterwards."""
    from src.config import cfg
    with restored_keys(cfg.task_arg, keys) as ta:
        ta.perturb = 0
        ta.mlp_dtype = "fp32"
        yield cfg


# --------------------------------------------------------------------------------------
# golden loaders
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g2():
    return np.load(os.path.join(HERE, "golden", "golden_v2.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def mg():
    return np.load(os.path.join(HERE, "golden", "golden_march_grad.npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def lego_grid():
    z = np.load(os.path.join(HERE, "golden", "lego_occupancy_grid.npz"))
    shape = tuple(int(v) for v in z["shape"])
    return torch.from_numpy(np.unpackbits(z["packed"])[: int(np.prod(shape))].reshape(shape).astype(bool))


@pytest.fixture(scope="module")
def trained_grid(g2):
    return torch.from_numpy(np.unpackbits(g2["bake128_packed"])[: 128 ** 3].reshape(128, 128, 128).astype(bool))


@pytest.fixture(scope="module")
def trained_state():
    z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _trained_net(cuda):
    from src.models.nerf.network import Network
    z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict({k: torch.from_numpy(z[k]) for k in z.files}, strict=True)
    return net.to(cuda)


# --------------------------------------------------------------------------------------
# the training march on the trained fixture net
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_net(cuda, g2, trained_grid):
    """The trained fixture net, its optimizer (the flat gradient), the 256 march rays, a ground truth."""
    from src.config import cfg
    from src.train.optimizer import make_optimizer
    old = {k: cfg.task_arg[k] for k in ("perturb", "mlp_dtype")}
    cfg.task_arg.perturb = 0
    cfg.task_arg.mlp_dtype = "fp32"
    net = _trained_net(cuda)
    opt = make_optimizer(cfg, net)
    rays = torch.from_numpy(g2["march_rays"]).to(cuda)
    t_table = torch.from_numpy(g2["march_t_table"]).to(cuda)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1)).to(cuda)
    yield {"net": net, "opt": opt, "rays": rays, "t_table": t_table, "gt": gt, "grid": trained_grid.to(cuda)}
    for k, v in old.items():
        cfg.task_arg[k] = v


def _batch(rays, cuda, rgbs=None, bg=None, device_scalar=False):
    """A batch as the loader makes it.  ``device_scalar``: near / far through ops.device_scalar (the cached device
    constants, no blocking copy) instead of torch.tensor."""
    from nerf_amd import ops
    near, far = ((ops.device_scalar(x, cuda) if device_scalar else torch.tensor([x], device=cuda)) for x in (2.0, 6.0))
    b = {"rays": torch.as_tensor(rays).to(cuda)[None], "near": near, "far": far}
    if rgbs is not None:
        b["rgbs"] = torch.as_tensor(rgbs).to(cuda)[None]
    if bg is not None:
        b["bg"] = torch.as_tensor(bg).to(cuda)[None]
    return b


def _march_grad(f, rays, dtype="fp32", **kw):
    from nerf_amd import ops
    kw.setdefault("t_table", f["t_table"])
    return ops.march_grad(f["net"].model_fine.packer(), rays, 2.0, 6.0, f["grid"], dtype=dtype, **kw)


def _loss(out, gt, rows=None):
    rgb, depth, acc = (out[m] if rows is None else out[m][:rows] for m in MAPS)
    gt = gt if rows is None else gt[:rows]
    return torch.nn.functional.mse_loss(rgb, gt) + 0.1 * depth.mean() + 0.1 * acc.mean()


def _flat_grad(f, loss):
    from nerf_amd import ops
    f["opt"].zero_grad()
    with ops.direct_grad():
        loss.backward()
    return f["opt"].flat_grad.clone()


def _write_grid(tmp_path, monkeypatch, grid):
    """logs/<cfg name>/occupancy_grid.pt under a temporary working directory."""
    from src.config.config import args
    monkeypatch.chdir(tmp_path)
    d = tmp_path / "logs" / os.path.splitext(os.path.basename(args.cfg_file))[0]
    d.mkdir(parents=True)
    torch.save(grid, str(d / "occupancy_grid.pt"))


def _trainer(cfg, cuda):
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    net = _trained_net(cuda)  # (torch.manual_seed(0): the renderer's seed follows torch.initial_seed())
    return net, make_trainer(cfg, net), make_optimizer(cfg, net)


# --------------------------------------------------------------------------------------
# the long-segment case of the distortion and background kernels' tests
# --------------------------------------------------------------------------------------
STEP = 0.005
INV_RANGE = 0.25  # near 2, far 6

SEG_LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 800, 4097, 4160]
LONG = (9, 10)                                # the segments past the backward's 64-chunk register window
ALPHA_ONE = [(8, 200), (10, 4100), (7, 64)]   # (segment, position): raw[3] = 1e4 -> alpha is exactly 1
SURPLUS = {6: 1, 7: 5}                        # segment -> length of its -1 tail
N_SEG = 23
N_TABLE = 5000


def long_segment_case():
    """23 segments, two of them past the backward's 64-chunk register window; alpha == 1 points, surplus tails;
    four cotangents (the fourth: of the distortion map)."""
    g = torch.Generator().manual_seed(5)
    lens = SEG_LENGTHS + torch.randint(0, 201, (N_SEG - len(SEG_LENGTHS),), generator=g).tolist()
    steps = []
    for i, n in enumerate(lens):
        s = torch.randperm(N_TABLE, generator=g)[:n].sort().values.to(torch.int32)  # strictly increasing
        if i in SURPLUS:
            s[n - SURPLUS[i]:] = -1
        steps.append(s)
    seg_off = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    M = int(seg_off[-1])
    raw = torch.randn(M, 4, generator=g)
    raw[:, :3] *= 2.0
    for i in range(N_SEG):  # sigma logits: x4 on half of the segments (the weights spread along the ray), x40 on the rest
        raw[int(seg_off[i]):int(seg_off[i + 1]), 3] *= 4.0 if i % 2 == 0 else 40.0
    for seg, pos in ALPHA_ONE:
        raw[int(seg_off[seg]) + pos, 3] = 1e4
    rays = torch.cat([torch.randn(N_SEG, 3, generator=g), torch.randn(N_SEG, 3, generator=g)], 1)
    cot = (torch.randn(N_SEG, 3, generator=g), torch.randn(N_SEG, generator=g), torch.randn(N_SEG, generator=g),
           torch.randn(N_SEG, generator=g))
    t_table = (2.0 + 0.005 * torch.arange(N_TABLE, dtype=torch.float64)).float()
    return dict(N=N_SEG, lens=lens, seg_off=seg_off, out_step=torch.cat(steps), raw=raw, rays=rays, cot=cot,
                t_table=t_table)


def _dist_double_sum(w, t):
    return INV_RANGE * ((w[:, None] * w[None, :] * (t[:, None] - t[None, :]).abs()).sum() + STEP / 3.0 * (w * w).sum())


def _dist_prefix(w, t):
    wt = w * t
    Wex, Sex = torch.cumsum(w, 0) - w, torch.cumsum(wt, 0) - wt
    return INV_RANGE * (2.0 * (w * (t * Wex - Sex)).sum() + STEP / 3.0 * (w * w).sum())


def _per_segment_bound(c, got, ref, what):
    """every entry within 1e-4 of its segment's largest reference entry"""
    off = c["seg_off"].tolist()
    worst = 0.0
    for r in range(c["N"]):
        if off[r + 1] == off[r]:
            continue
        big = float(ref[off[r]:off[r + 1]].abs().max())
        err = float((got[off[r]:off[r + 1]].double() - ref[off[r]:off[r + 1]]).abs().max())
        worst = max(worst, err / big if big > 0 else (0.0 if err == 0 else float("inf")))
        assert err <= 1e-4 * big, (what, r, c["lens"][r], err, big)
    return worst


# --------------------------------------------------------------------------------------
# the background blend
# --------------------------------------------------------------------------------------
def blend_f32(rgba, bg):
    """The kernel's blend in numpy: fadd(fmul(C, a), fmul(fsub(1, a), bg)), every op rounded to fp32."""
    rgba, bg = np.asarray(rgba, np.float32), np.asarray(bg, np.float32)
    a = rgba[..., 3:4]
    left = (np.float32(1.0) - a).astype(np.float32)
    out = ((rgba[..., :3] * a).astype(np.float32) + (left * bg).astype(np.float32)).astype(np.float32)
    assert out.dtype == np.float32
    return out
