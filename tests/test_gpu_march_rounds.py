"""The round march on the GPU (csrc/march.hip: init, gather, composite, finish), the MLP out of the loop.

The raw value of a gathered point comes from a synthetic field by (out_ray, out_step); the scene, the fp64
reference and the driver are tests/march_rounds_ref.py (its CPU-side claims: tests/test_march_rounds_cpu.py).

  A  against fp64: the maps on every kept ray, ray_used exactly, the counters, the exact cases
  B  bit-invariance under the round structure: K, k_low, t_split, k_low_grow, the buffer size, one / two pass,
     the macro grid change speed only -- one thread composites a ray in step order with separately rounded fp32
     operations, so the maps, T, ray_used and consumed are bit-identical
  C  the per-round contract of gather and composite, from snapshots of every round
  D  row independence: the first 1, 64, 65 rays alone
  E  the production loop, ops.march, on the trained fixture net under the same kinds of options

Measured on the MI355X, part A, the worst error on the kept rays over both walks, both thresholds and both
backgrounds: rgb 6.9e-7, acc 6.6e-7 (bound 1e-5), depth 2.8e-6 (bound 5e-5); 4 and 6 rays left out at t_thresh
1e-4, none at 0.  The default options take 13 rounds here (36,983 points evaluated for 34,521 composited), K = 1
takes 508, cap = N K / 4 with K = 12 about 64 with 230 rays waiting in the first.
"""
import pytest
import torch

import march_rounds_ref as R
from march_support import fixture_net, g2, trained_grid  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BITS = ("rgb", "depth", "acc", "T", "ray_used")


@pytest.fixture(scope="module")
def scene():
    return R.make_scene()


@pytest.fixture(scope="module")
def runs(scene, cuda):
    """run(name, shifted, ...): run_rounds under a configuration of R.CONFIGS, computed once and shared."""
    cache = {}

    def run(name, shifted, t_thresh=R.T_THRESH, white=True, snapshots=False, **over):
        key = (name, shifted, t_thresh, white, snapshots, tuple(sorted(over.items())))
        if key not in cache:
            o = R.resolve(scene, {**R.CONFIGS[name], **over}, shifted)
            cache[key] = (o, R.run_rounds(scene, t_shift=shifted, t_thresh=t_thresh, white=white,
                                          snapshots=snapshots, device=cuda, **o))
        return cache[key]
    return run


def _assert_ended(out):
    assert not bool(out["alive"].any())
    assert out["evaluated"] == out["evaluated_host"] >= out["consumed"] == int(out["ray_used"].sum())
    for k in ("rgb", "depth", "acc", "T"):
        assert not bool(torch.isnan(out[k]).any()), k


# --------------------------------------------------------------------------------------
# A. against fp64
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("white", [True, False])
@pytest.mark.parametrize("t_thresh", [R.T_THRESH, 0.0])
@pytest.mark.parametrize("shifted", [False, True])
def test_against_fp64(scene, runs, shifted, t_thresh, white):
    _, out = runs("default", shifted, t_thresh, white)
    ref = R.reference(scene, shifted, t_thresh, white)
    keep = ~ref["near"]
    assert int((~keep).sum()) <= R.MAX_LEFT_OUT
    err = {k: float((out[k].double() - ref[k])[keep].abs().max()) for k in ("rgb", "acc", "depth")}
    print(f"\nshift {shifted}, t_thresh {t_thresh}, white {white}: worst error on the {int(keep.sum())} kept rays "
          f"rgb {err['rgb']:.2e}, acc {err['acc']:.2e} (bound 1e-5), depth {err['depth']:.2e} (bound 5e-5); "
          f"{out['rounds']} rounds, {out['evaluated']} points evaluated for {out['consumed']} composited")
    _assert_ended(out)
    used = out["ray_used"].long()
    assert torch.equal(used[keep], ref["used"][keep])
    assert bool(((used - ref["used"]).abs() <= 1).all())
    assert err["rgb"] <= 1e-5 and err["acc"] <= 1e-5 and err["depth"] <= 5e-5, err
    bg = 1.0 if white else 0.0
    c0 = scene["cls"] == 0  # sigma <= 0 everywhere: ends by exhaustion with acc == 0, the background exactly
    assert bool((out["acc"][c0] == 0).all()) and bool((out["rgb"][c0] == bg).all()) and bool((out["T"][c0] == 1).all())
    assert torch.equal(used[c0], scene["walk"][shifted]["count"][c0])
    none = scene["walk"][shifted]["count"] == 0
    assert int(none.sum()) >= 3
    assert bool((out["rgb"][none] == bg).all()) and bool((out["depth"][none] == 0).all())
    assert bool((out["acc"][none] == 0).all()) and bool((used[none] == 0).all())
    if t_thresh == 0.0:  # nothing terminates: every occupied step is composited, on through T == 0
        assert torch.equal(used, scene["walk"][shifted]["count"])
        assert int((out["T"] == 0).sum()) >= 3


# --------------------------------------------------------------------------------------
# B. bit-invariance under the round structure
# --------------------------------------------------------------------------------------
B_CASES = [(name, R.T_THRESH) for name in R.CONFIGS if name != "default"]
B_CASES += [("k5", 0.0), ("tight_sched", 0.0), ("tight_sched_two_pass", 0.0)]


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name,t_thresh", B_CASES)
def test_round_structure_changes_no_bit(scene, runs, name, t_thresh, shifted):
    _, base = runs("default", shifted, t_thresh)
    o, out = runs(name, shifted, t_thresh)
    n = o.get("n_rays") or scene["N"]
    print(f"\n{name}, shift {shifted}, t_thresh {t_thresh}: {out['rounds']} rounds (default {base['rounds']}), "
          f"{out['evaluated']} points evaluated (default {base['evaluated']})")
    _assert_ended(out)
    for k in BITS:
        assert torch.equal(out[k], base[k][:n]), k
    assert out["consumed"] == int(base["ray_used"][:n].sum())
    if n == scene["N"]:
        assert out["consumed"] == base["consumed"]
    if o["cap"] < n * min(o["k_schedule"]):  # a tight buffer: rays waited, so there were more rounds than their own
        assert out["evaluated"] >= out["consumed"] and out["rounds"] > 1


@pytest.mark.parametrize("shifted", [False, True])
def test_full_quota_ray_ends_a_round_later_with_nothing(scene, runs, shifted):
    """K = c*, the occupied count of ray r*, which has empty steps after its last occupied one: round one gathers
    all of it and stops on the quota (exhausted == 0, the ray stays alive); round two walks to the end of the
    table, gathers nothing and ends the ray."""
    r, c = R.pick_cstar(scene, shifted)
    o, out = runs("kcstar", shifted, snapshots=True)
    assert o["k_schedule"] == (c,)
    w = scene["walk"][shifted]
    s1, s2 = out["snaps"][0], out["snaps"][1]
    assert s1["K"] == c and int(s1["gather"]["ray_cnt"][r]) == c and int(s1["gather"]["exhausted"][r]) == 0
    assert int(s1["gather"]["next_step"][r]) == int(w["occ_steps"][r, c - 1]) + 1 < scene["S"]
    assert int(s1["after"]["alive"][r]) == 1 and int(s1["after"]["ray_used"][r]) == c
    assert int(s2["before"]["alive"][r]) == 1
    assert int(s2["gather"]["ray_cnt"][r]) == 0 and int(s2["gather"]["exhausted"][r]) == 1
    assert int(s2["gather"]["next_step"][r]) == scene["S"]
    assert int(s2["after"]["alive"][r]) == 0 and int(s2["after"]["ray_used"][r]) == c
    assert torch.equal(s2["after"]["T"][r], s1["after"]["T"][r])
    _, base = runs("default", shifted)
    for k in BITS:
        assert torch.equal(out[k], base[k]), k


# --------------------------------------------------------------------------------------
# C. the per-round contract
# --------------------------------------------------------------------------------------
def _check_round(scene, shifted, o, t_thresh, snap):
    w = scene["walk"][shifted]
    N, S, cap = o.get("n_rays") or scene["N"], scene["S"], o["cap"]
    rows = torch.arange(N)
    count, occ_steps = w["count"][:N], w["occ_steps"][:N]
    b, g, a = snap["before"], snap["gather"], snap["after"]
    K, kl, n = snap["K"], snap["k_low"], snap["n"]
    reserved, entered = snap["counters"]
    live = b["alive"].bool()
    assert entered == int(live.sum())
    assert n == min(reserved, cap)
    # what every live ray must have asked for: its quota (from its T before the round) or what is left of it
    s0 = b["next_step"].long()
    assert bool(((s0 >= 0) & (s0 <= S)).all())
    rank0 = w["rank"][rows, s0]
    quota = torch.where(b["T"] < torch.tensor(o["t_split"], dtype=torch.float32), kl, K)
    want = torch.minimum(quota, count - rank0) * live
    assert int(want.sum()) == reserved
    off, cnt = g["ray_off"].long(), g["ray_cnt"].long()
    # the reservations tile [0, reserved): no gap, no overlap
    asked = torch.nonzero(want > 0).flatten()
    asked = asked[torch.argsort(off[asked])]
    if asked.numel():
        ends = off[asked] + want[asked]
        assert int(off[asked[0]]) == 0 and torch.equal(off[asked][1:], ends[:-1]) and int(ends[-1]) == reserved
    assert bool((cnt[~live] == 0).all())
    over = live & (off + want > cap)
    fits = live & ~over
    assert torch.equal(cnt[fits], want[fits])
    # a ray that finds no room: the part of its reservation below cap is written (ray_cnt = minus that many),
    # its position and its exhausted flag are left alone
    assert torch.equal(cnt[over], -torch.minimum((cap - off).clamp(min=0), want)[over])
    keep = ~fits
    assert torch.equal(g["next_step"][keep], b["next_step"][keep])
    assert torch.equal(g["exhausted"][keep], b["exhausted"][keep])
    # a ray that fits: stopped on its quota (the step after its last point) or at the end of the table
    # (exhausted: the walk stands at the end of the table -- also when the quota's last point is the last step)
    nxt = torch.where(want == quota, occ_steps[rows, (rank0 + want - 1).clamp(min=0)] + 1, torch.full_like(want, S))
    assert torch.equal(g["next_step"][fits].long(), nxt[fits])
    assert torch.equal(g["exhausted"][fits].bool(), (nxt == S)[fits])
    # the points: every position below n written once, with its ray's next occupied steps in order
    nw = cnt.abs()
    assert int(nw.sum()) == n
    ray = torch.repeat_interleave(rows, nw)
    j = torch.arange(n) - torch.repeat_interleave(torch.cumsum(nw, 0) - nw, nw)
    pos = off[ray] + j
    assert torch.equal(torch.sort(pos).values, torch.arange(n))
    step = occ_steps[ray, rank0[ray] + j]
    assert bool((step < S).all())
    assert torch.equal(g["out_ray"][pos].long(), ray) and torch.equal(g["out_step"][pos].long(), step)
    assert bool(w["occ"][g["out_ray"][:n].long(), g["out_step"][:n].long()].all())
    assert torch.equal(g["out_pts"][pos], w["pts"][ray, step])
    # nothing at or past n is written
    assert bool((g["out_ray"][n:] == -1).all()) and bool((g["out_step"][n:] == -1).all())
    assert bool(torch.isnan(g["out_pts"][n:]).all())
    # composite: a live ray is dead afterwards iff it terminated or was exhausted; the others keep their state
    term = live & (a["T"] < torch.tensor(t_thresh, dtype=torch.float32))
    assert torch.equal(~a["alive"].bool(), ~live | term | (live & g["exhausted"].bool()))
    idle = ~live | (cnt <= 0)
    assert torch.equal(a["T"][idle], b["T"][idle])
    d = (a["ray_used"] - b["ray_used"]).long()
    got = cnt.clamp(min=0)
    assert bool((d[idle] == 0).all()) and bool((d <= got).all()) and bool((d[got > 0] >= 1).all())
    assert torch.equal(d[~term], got[~term])
    return int((over & (want > 0)).sum())


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", ["default", "tight_sched", "tight_sched_two_pass", "tight_k12"])
def test_per_round_contract(scene, runs, name, shifted):
    o, out = runs(name, shifted, snapshots=True)
    waited = [_check_round(scene, shifted, o, R.T_THRESH, s) for s in out["snaps"]]
    assert out["snaps"][-1]["counters"] == [0, 0] and len(out["snaps"]) == out["rounds"] + 1
    print(f"\n{name}, shift {shifted}: {out['rounds']} rounds, rays that waited per round {waited}")
    if name == "default":
        assert sum(waited) == 0
    else:  # three quarters of the rays wait in the first round
        assert waited[0] >= scene["N"] // 2
    _, base = runs("default", shifted)
    for k in BITS:
        assert torch.equal(out[k], base[k]), k


# --------------------------------------------------------------------------------------
# D. row independence
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65])  # one lane, one full wave, a wave and one lane
def test_first_rays_alone(scene, runs, n, shifted):
    _, base = runs("default", shifted)
    _, out = runs("default", shifted, n_rays=n)
    _assert_ended(out)
    for k in BITS:
        assert out[k].shape[0] == n and torch.equal(out[k], base[k][:n]), k
    assert out["consumed"] == int(base["ray_used"][:n].sum())


# --------------------------------------------------------------------------------------
# E. the production loop
# --------------------------------------------------------------------------------------
def _production(f, **kw):
    from nerf_amd import ops
    with torch.no_grad():
        out = ops.march(f["net"].model_fine.packer(), f["rays"], 2.0, 6.0, f["grid"], dtype="fp32", return_used=True,
                        **kw)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def production_base(fixture_net):
    return _production(fixture_net)


@pytest.mark.parametrize("opts", [dict(round_bytes=36 * 1024), dict(k_schedule=(5,)), dict(k_low=1, t_split=2.0),
                                  dict(k_low_grow=0), dict(sync_every=1), dict(sync_every=7), dict(one_pass=False),
                                  dict(use_macro=False)], ids=lambda o: "-".join(f"{k}={v}" for k, v in o.items()))
def test_ops_march_round_options_change_no_bit(fixture_net, g2, production_base, opts):
    """ops.march on the trained fixture net: this relies on an MLP row's bits not depending on its position in
    the launch (test_gpu_kernels.py::test_mlp_rows_independent_of_position)."""
    base = production_base
    assert base["n_queried"] == int(g2["march_queried"]) == int(base["ray_used"].sum())
    assert base["n_evaluated"] >= base["n_queried"]
    out = _production(fixture_net, **opts)
    print(f"\n{opts}: {out['rounds']} rounds (default {base['rounds']}), {out['n_evaluated']} points evaluated "
          f"(default {base['n_evaluated']}) for {out['n_queried']} composited")
    for k in ("rgb_map_f", "depth_map_f", "acc_map_f", "ray_used"):
        assert torch.equal(out[k], base[k]), k
    assert out["n_queried"] == base["n_queried"]
    assert out["n_evaluated"] >= out["n_queried"]
    if "round_bytes" in opts:  # 1024 points for 256 rays x K = 12: the buffer overflows every early round
        assert out["rounds"] > base["rounds"]
