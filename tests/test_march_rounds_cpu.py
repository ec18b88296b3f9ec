"""The round-march tests' scene, reference and round model (tests/march_rounds_ref.py), without a GPU.

What tests/test_gpu_march_rounds.py relies on is asserted here: the scene holds every edge class, few rays are
left out of the fp64 comparisons, the reference restated in fp32 torch agrees with fp64 well inside the bounds the
kernels are held to, and a plain-Python model of the round loop ends within the driver's round bound for every
configuration the GPU tests run.
"""
import pytest
import torch

import march_rounds_ref as R


@pytest.fixture(scope="module")
def scene():
    return R.make_scene()


def test_scene_anchor(scene):
    """The counts of the prototype scene, loosely: a changed draw may move them, not change their kind."""
    assert scene["N"] == 321 and scene["S"] == 800 and scene["grid"].shape == (32, 32, 32)
    cells = int(scene["grid"].sum())
    assert 1800 <= cells <= 3000, cells
    macro = scene["grid"].reshape(4, 8, 4, 8, 4, 8).any(5).any(3).any(1)
    assert 16 <= int((~macro).sum()) <= 48, int((~macro).sum())  # about half of the 4^3 macro blocks empty
    for shifted in (False, True):
        count = scene["walk"][shifted]["count"]
        print(f"\nshift {shifted}: occupied steps per ray {int(count.min())} / {float(count.float().median()):.0f} / "
              f"{int(count.max())} (min / median / max), {int((count == 0).sum())} rays with none, "
              f"{int(count.sum())} in all")
        assert int(count.min()) == 0 and int(count.max()) > 400 and 100 <= float(count.float().median()) <= 250
        assert 30000 <= int(count.sum()) <= 90000
    assert float(scene["t_shift"].min()) >= 0.0 and float(scene["t_shift"].max()) < R.STEP
    # the two walks differ (the shift moves steps across cell boundaries)
    assert not torch.equal(scene["walk"][False]["occ"], scene["walk"][True]["occ"])


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("t_thresh", [R.T_THRESH, 0.0])
def test_leave_out_cap(scene, shifted, t_thresh):
    ref = R.reference(scene, shifted, t_thresh)
    left = int(ref["near"].sum())
    print(f"\nshift {shifted}, t_thresh {t_thresh}: {left} rays left out of the fp64 comparisons")
    assert left <= R.MAX_LEFT_OUT
    if t_thresh == 0.0:  # nothing terminates: every occupied step is composited, on through T == 0
        assert left == 0 and not bool(ref["terminated"].any())
        assert torch.equal(ref["used"], scene["walk"][shifted]["count"])


@pytest.mark.parametrize("shifted", [False, True])
def test_scene_holds_every_edge_class(scene, shifted):
    w = scene["walk"][shifted]
    ref = R.reference(scene, shifted)
    count, used, term, cls = w["count"], ref["used"], ref["terminated"], scene["cls"]
    S = scene["S"]
    last = torch.where(count > 0, w["occ_steps"].gather(1, (count - 1).clamp(min=0)[:, None])[:, 0],
                       torch.full_like(count, S))
    classes = {
        "no occupied step": count == 0,
        "exhaustion without termination": (count > 0) & ~term,
        "termination at exactly point 12": term & (used == 12) & (cls == 4),
        "termination at exactly point 13": term & (used == 13) & (cls == 4),
        "final T == 0": ref["T"] == 0,
        "empty steps after the last occupied one": (count > 0) & (last < S - 1),
        "early termination": term & (used < count),
        "class-0 rays": (cls == 0) & (count > 0),
    }
    n = {k: int(v.sum()) for k, v in classes.items()}
    print(f"\nshift {shifted}: {n}; {int(used.sum())} of {int(count.sum())} points composited")
    for k, v in n.items():
        assert v >= 3, (k, v)
    # the two rays that miss the box have no occupied step; a class-0 ray ends with acc == 0 and white rgb 1
    assert int(count[-1]) == 0 and int(count[-2]) == 0
    c0 = cls == 0
    assert bool((ref["acc"][c0] == 0).all()) and bool((ref["rgb"][c0] == 1).all()) and not bool(term[c0].any())
    # the 1e4 point sits where the construction says: -1 before it, on the ray's 12th / 13th occupied step
    for r in torch.nonzero((cls == 4) & (count > 12)).flatten().tolist():
        j = 11 if r % 2 == 0 else 12
        sig = w["field"][r, w["occ_steps"][r, :j + 1], 3]
        assert bool((sig[:j] == -1).all()) and float(sig[j]) == 1e4 and int(used[r]) == j + 1 and bool(term[r])
    r_star, c_star = R.pick_cstar(scene, shifted)
    print(f"r* = {r_star}, c* = {c_star}")
    assert int(count[r_star]) == c_star >= 64 and not bool(term[r_star]) and int(last[r_star]) < S - 1
    assert int(used[r_star]) == c_star


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("t_thresh", [R.T_THRESH, 0.0])
def test_reference_in_fp32_agrees_with_fp64(scene, shifted, t_thresh):
    """The same loop in fp32 torch: the fp64 `used` on every kept ray, the maps within the march's bounds of
    test_render_accelerated_real_grid (1e-5 rgb / acc, 5e-5 depth) -- the reference alone sits well inside them."""
    r64 = R.reference(scene, shifted, t_thresh)
    r32 = R.reference(scene, shifted, t_thresh, dtype=torch.float32)
    keep = ~r64["near"]
    assert r32["rgb"].dtype == torch.float32
    assert torch.equal(r32["used"][keep], r64["used"][keep])
    assert bool(((r32["used"] - r64["used"]).abs() <= 1).all())
    err = {k: float((r32[k].double() - r64[k])[keep].abs().max()) for k in ("rgb", "acc", "depth")}
    print(f"\nshift {shifted}, t_thresh {t_thresh}: fp32 loop against fp64, worst {err}")
    assert err["rgb"] <= 1e-5 and err["acc"] <= 1e-5 and err["depth"] <= 5e-5, err


@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("name", list(R.CONFIGS))
def test_round_model_ends_within_the_bound(scene, shifted, name):
    """The quota from T < t_split, the k_low growth, the rays served in index order against cap: the model of the
    round loop ends within the bound the GPU driver loops over, for every configuration the GPU tests run."""
    o = R.resolve(scene, R.CONFIGS[name], shifted)
    N = o.get("n_rays") or scene["N"]
    count = scene["walk"][shifted]["count"][:N]
    assert o["cap"] >= 1
    bound = R.round_bound(count, o["k_schedule"], o["k_low"], o["cap"])
    for t_thresh in (R.T_THRESH, 0.0):
        rounds, evaluated = R.model_rounds(scene, shifted, t_thresh=t_thresh, **o)
        used = int(R.reference(scene, shifted, t_thresh, n_rays=o.get("n_rays"))["used"].sum())
        print(f"\n{name}, shift {shifted}, t_thresh {t_thresh}: {rounds} rounds (bound {bound}), "
              f"{evaluated} points evaluated for {used} composited")
        assert rounds + 1 <= bound
        assert evaluated >= used
        assert rounds <= 700, rounds  # (what keeps a GPU case at a few seconds)
