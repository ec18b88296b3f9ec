"""CPU: the point budget's host side (task_arg.point_budget) -- the configuration keys and their
validation, the RayBudget controller's integer formula on hand-made cases, its convergence on a
synthetic stream, its state round trip, and the C ABI's argument checks of nerf_march_budget (no
kernel launches, no GPU)."""
import ctypes
import math
import os
import re

import pytest

from march_support import lib, restored_keys

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = {"target": 0, "max_points": 0, "min_rays": 1024, "max_rays": 32768, "granularity": 256}
GRID_DEFAULTS = {"interval": 16, "warmup_updates": 16, "period": 4, "decay": 0.95, "seed": 0}
INT32_MAX = 2 ** 31 - 1


def formula(n_rays, n_queried, target, min_rays=1024, max_rays=32768, granularity=256):
    """The issue's formula, restated."""
    want = max_rays if n_queried == 0 else (target * n_rays) // n_queried
    want = min(max(want, n_rays // 2), 2 * n_rays)
    return min(max((want // granularity) * granularity, min_rays), max_rays)


@pytest.fixture()
def task_arg():
    """cfg.task_arg with the keys this file touches restored afterwards."""
    from src.config import cfg
    keys = ("train_renderer", "train_grid", "grid_update", "point_budget", "train_rays")
    with restored_keys(cfg.task_arg, keys) as ta:
        yield ta


# --------------------------------------------------------------------------------------
# configuration
# --------------------------------------------------------------------------------------
def test_defaults_are_in_the_config_and_off(task_arg, tmp_path, monkeypatch):
    from src.models.nerf.renderer import ray_budget as rb
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    assert dict(task_arg.point_budget) == rb.DEFAULTS == DEFAULTS
    assert dict(task_arg.grid_update) == GRID_DEFAULTS  # (the neighbouring node is as it was)
    assert rb.point_budget_settings(task_arg) == DEFAULTS
    assert rb.RayBudget.from_config(task_arg) is None
    w = NetworkWrapper(None)  # target 0: today's wrapper
    assert w.ray_budget is None and w.renderer.max_points is None and w.online_grid is None
    node = task_arg.pop("point_budget")  # a configuration without the node: the same defaults
    try:
        assert rb.point_budget_settings(task_arg) == DEFAULTS and rb.RayBudget.from_config(task_arg) is None
        assert NetworkWrapper(None).ray_budget is None
    finally:
        task_arg.point_budget = node
    assert rb.march_steps(task_arg.near, task_arg.far, task_arg.render_step_size) == 800


def test_wrapper_owns_a_budget_and_sets_the_loader(task_arg, tmp_path, monkeypatch):
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    task_arg.train_renderer = "accelerated"
    task_arg.train_grid = "online"
    task_arg.point_budget = {"target": 262144}
    w = NetworkWrapper(None)
    b = w.ray_budget
    assert (b.target, b.max_points, b.min_rays, b.max_rays, b.granularity) == (262144, 524288, 1024, 32768, 256)
    assert b.rays == int(task_arg.train_rays) == 4096 and b.observations == 0
    assert w.renderer.max_points == 524288 and w.online_grid is not None

    class Loader:
        class dataset:
            batch_rays = 4096

    task_arg.train_rays = 5000  # starts at train_rays, clamped and rounded the same way
    task_arg.point_budget = {"target": 262144, "max_points": 300000}
    w = NetworkWrapper(None, Loader)
    assert w.ray_budget.rays == 4864 == Loader.dataset.batch_rays and w.ray_budget.max_points == 300000
    task_arg.train_rays = 100
    assert NetworkWrapper(None).ray_budget.rays == 1024
    task_arg.train_rays = 10 ** 6
    assert NetworkWrapper(None).ray_budget.rays == 32768


@pytest.mark.parametrize("renderer,node,match", [
    ("hierarchical", {"target": 65536}, r"point_budget\.target"),
    ("accelerated", {"target": 65536, "max_points": 799}, r"point_budget\.max_points"),
    ("accelerated", {"target": 300}, r"point_budget\.max_points"),  # the default cap, 2 * target = 600 < 800 steps
    ("accelerated", {"target": 65536, "min_rays": 1000}, r"point_budget\.min_rays"),
    ("accelerated", {"target": 65536, "max_rays": 32767}, r"point_budget\.max_rays"),
    ("accelerated", {"target": 65536, "granularity": 100}, r"point_budget\.min_rays"),
    ("accelerated", {"target": 65536, "min_rays": 2048, "max_rays": 1024}, r"point_budget\.min_rays"),
    ("accelerated", {"target": -1}, r"point_budget\.target"),
    ("accelerated", {"target": 2.5}, r"point_budget\.target"),
    ("accelerated", {"target": 65536, "granularity": 0}, r"point_budget\.granularity"),
    ("accelerated", {"target": 65536, "max_points": 2 ** 31}, r"point_budget\.max_points"),
    ("accelerated", {"target": 65536, "rays": 4096}, "unknown key"),
])
def test_validation_names_the_key(task_arg, tmp_path, monkeypatch, renderer, node, match):
    from src.models.nerf.renderer.ray_budget import RayBudget
    from src.train.trainers.nerf import NetworkWrapper
    monkeypatch.chdir(tmp_path)
    task_arg.train_renderer = renderer
    task_arg.train_grid = "online" if renderer == "accelerated" else "file"
    task_arg.point_budget = node
    with pytest.raises(ValueError, match=match):
        RayBudget.from_config(task_arg)
    with pytest.raises(ValueError, match=match):
        NetworkWrapper(None)


def test_a_cap_of_exactly_the_steps_is_accepted(task_arg):
    from src.models.nerf.renderer.ray_budget import RayBudget
    task_arg.train_renderer = "accelerated"
    task_arg.point_budget = {"target": 400, "max_points": 800}
    assert RayBudget.from_config(task_arg).max_points == 800
    task_arg.point_budget = {"target": 400}  # 2 * target
    assert RayBudget.from_config(task_arg).max_points == 800


# --------------------------------------------------------------------------------------
# the formula
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rays,n_queried,want", [
    (4096, 0, 8192),          # nothing queried: max_rays, limited to twice this step's count
    (16384, 0, 32768),        # ... which reaches max_rays itself
    (4096, 100000, 2560),     # 65536 * 4096 // 100000 = 2684: within the factor 2, rounded down
    (4096, 4096 * 4, 8192),   # 16384 rays wanted: the factor 2 upwards
    (4096, 4096 * 200, 2048),  # 327 rays wanted: the factor 2 downwards
    (4096, 4096 * 13, 4864),  # 5041 rays wanted: rounded down to a multiple of 256
    (4096, 4096 * 16, 4096),  # exactly on a multiple
    (1024, 1024 * 400, 1024),  # 163 wanted, half is 512: the lower clamp
    (32768, 32768, 32768),    # 65536 wanted, twice is 65536: the upper clamp
    (256, 256 * 16, 1024),    # a batch below min_rays (a caller's own): twice is 512, clamped up
])
def test_observe_hand_made(n_rays, n_queried, want):
    from src.models.nerf.renderer.ray_budget import RayBudget
    b = RayBudget(65536, train_rays=4096)
    assert b.observe(n_rays, n_queried) == want == b.rays == formula(n_rays, n_queried, 65536)
    assert b.observations == 1


def test_observe_other_bounds():
    from src.models.nerf.renderer.ray_budget import RayBudget
    b = RayBudget(8192, max_points=4096, min_rays=300, max_rays=900, granularity=100, train_rays=256, n_steps=800)
    assert b.rays == 300 and b.max_points == 4096  # 256 -> 200 -> clamped to min_rays
    assert b.observe(256, 13382) == 300 == formula(256, 13382, 8192, 300, 900, 100)  # 156 wanted
    assert b.observe(600, 600 * 11) == 700  # 8192 // 11 = 744 -> 700
    assert b.observe(600, 600) == 900  # 8192 wanted, twice is 1200 -> the upper clamp
    assert b.observations == 3


def test_convergence_on_a_fixed_stream():
    """The per-ray counts are a fixed array (ray i always costs c[i] points; a batch of n rays is its first
    n), starting at min_rays: the count reaches the formula's fixed point within ceil(log2(fixed point /
    start)) + 1 steps -- the doublings, then one step that lands -- and stays there."""
    from src.models.nerf.renderer.ray_budget import RayBudget
    target = 262144
    c = [20 + (i * 7) % 13 for i in range(32768)]  # mean ~26 points per ray
    prefix = [0]
    for v in c:
        prefix.append(prefix[-1] + v)
    fixed = 1024
    for _ in range(100):
        nxt = formula(fixed, prefix[fixed], target)
        if nxt == fixed:
            break
        fixed = nxt
    assert formula(fixed, prefix[fixed], target) == fixed and 1024 < fixed < 32768
    assert abs(prefix[fixed] - target) < 0.05 * target  # (the fixed point does sit at the target)
    b = RayBudget(target, train_rays=0)
    assert b.rays == 1024
    bound = math.ceil(math.log2(fixed / 1024)) + 1
    traj = []
    for _ in range(bound + 10):
        traj.append(b.observe(b.rays, prefix[b.rays]))
    assert fixed in traj and traj.index(fixed) + 1 <= bound, (traj, fixed, bound)
    assert all(v == fixed for v in traj[traj.index(fixed):]), traj
    assert all(b2 <= 2 * a for a, b2 in zip([1024] + traj, traj))


def test_state_round_trip(tmp_path):
    import torch
    from src.models.nerf.renderer.ray_budget import RayBudget
    a = RayBudget(65536, train_rays=4096)
    for _ in range(3):
        a.observe(a.rays, a.rays * 9)  # 9 points a ray: 7281 rays wanted
    assert (a.rays, a.observations) == (7168, 3)
    sd = a.state_dict()
    assert sd == {"rays": 7168, "observations": 3}
    path = str(tmp_path / "ray_budget_state.pt")
    torch.save(sd, path)
    b = RayBudget(65536, train_rays=4096)
    b.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))  # plain data: no unpickled code
    assert (b.rays, b.observations) == (7168, 3)
    assert b.observe(b.rays, 7168 * 8) == a.observe(a.rays, 7168 * 8) == 8192
    with pytest.raises(ValueError, match="ray budget state"):  # a count this run's bounds do not allow
        RayBudget(65536, max_rays=4096, train_rays=4096).load_state_dict(sd)


def test_the_module_needs_no_torch():
    src = open(os.path.join(ROOT, "nerf-replication_amd", "src", "models", "nerf", "renderer", "ray_budget.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(torch|numpy|nerf_amd)", src, flags=re.M)


# --------------------------------------------------------------------------------------
# C ABI
# --------------------------------------------------------------------------------------
def test_header_and_signature_have_the_entry_point(lib):
    from nerf_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nerf_amd.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+nerf_march_budget\s*\(([^)]*)\)\s*;", text)
    assert m, "nerf_march_budget is not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["const int32_t* ray_used", "int64_t N", "int64_t budget", "int32_t* seg_off", "int64_t* keep",
                      "hipStream_t stream"]
    res, args = _lib.SIGNATURES["nerf_march_budget"]
    assert res is ctypes.c_int and len(args) == len(params)
    assert args[1] is ctypes.c_int64 and args[2] is ctypes.c_int64
    assert hasattr(lib, "nerf_march_budget")
    assert lib.nerf_abi_version() == 4  # additions do not bump it


def test_argument_errors_without_gpu(lib):
    from nerf_amd._lib import check
    d = ctypes.c_void_p(16)  # never dereferenced: the argument checks come first

    def budget(used=d, n=64, b=1000, seg=d, keep=d):
        return lib.nerf_march_budget(used, n, b, seg, keep, None)

    for bad, match in ((dict(b=-1), "budget must be in"), (dict(b=INT32_MAX + 1), "budget must be in"),
                       (dict(b=2 ** 40), "budget must be in"), (dict(seg=None), "null pointer"),
                       (dict(keep=None), "null pointer"), (dict(used=None), "null pointer"),
                       (dict(n=-1), "N must be")):
        assert budget(**bad) == -22, bad
        with pytest.raises(RuntimeError, match=match):
            check(budget(**bad), "nerf_march_budget")


def test_march_grad_rejects_a_cap_below_the_steps():
    """Checked before anything touches the device."""
    import torch
    from nerf_amd import ops
    for cap in (799, 0, -5, 2 ** 31):
        with pytest.raises(ValueError, match="max_points"):
            ops.march_grad(None, torch.zeros(4, 6), 2.0, 6.0, torch.ones(8, 8, 8, dtype=torch.bool), max_points=cap)
