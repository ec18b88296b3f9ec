"""Jittered march steps on the GPU (task_arg.train_march_jitter; nerf_march_jitter and the *_shift
entry points).

The reference for "shifted" behaviour is the already-pinned code run on a shifted table: for rays that
share a shift c, the new path must equal today's path called with t_table + c (fp32, c a float32),
because fadd(t_table[k], c) is that table's entry.  Checked here:

  1. the draw against a NumPy restatement of Philox-4x32-10, bit for bit;
  2. the walk (empty-space skip included) against a brute-force occupancy test of every shifted step;
  3. a null shift == a shift of zeros; groups of rays sharing a shift == the shifted table, bit for bit
     (the march and the segment compositing pair);
  4. the segment kernels with per-ray shifts against fp64;
  5. the gradient end to end: one shift for all rays == the shifted table, bit for bit; reproducible;
  6. under a point budget the shift is cut with the rays;
  7. the trainer: the key on (one draw per step, reproducible, chunk-independent), off (nothing drawn),
     and no jitter without grad;
  8. it trains.
"""
import os

import numpy as np
import pytest
import torch

from march_support import (MAPS, _batch, _flat_grad, _loss, _march_grad, _trained_net, _trainer, _write_grid,
                           fixture_net, fp32_cfg, g2, lego_grid, trained_grid)

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
STEP = np.float32(0.005)
BELOW_STEP = np.nextafter(STEP, np.float32(0))  # the largest shift below a step
GROUP_SHIFTS = [np.float32(0), np.float32(0.00125), np.float32(0.0025), BELOW_STEP]


@pytest.fixture()
def jcfg():
    """cfg with the keys the tests below set restored afterwards."""
    yield from fp32_cfg(("train_renderer", "train_grid", "train_march_jitter", "point_budget", "mlp_dtype",
                         "perturb", "chunk_size"))


def _random_shifts(n, seed):
    """float32 in [0, step); ray 0 gets 0, ray 1 the largest value below a step."""
    s = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) * float(STEP)).to(torch.float32)
    s = s.clamp(max=float(BELOW_STEP))
    s[0] = 0.0
    s[1] = float(BELOW_STEP)
    assert float(s.min()) == 0.0 and float(s.max()) == float(BELOW_STEP) < float(STEP)
    return s


def _same(a, b, keys=None):
    for k in (keys or a):
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


# --------------------------------------------------------------------------------------
# 1. the draw
# --------------------------------------------------------------------------------------
def _philox_first_word(n, seed, offset):
    """Philox-4x32-10, counter (idx lo, idx hi, offset lo, offset hi), key (seed lo, seed hi): word 0."""
    mask = np.uint64(0xFFFFFFFF)
    sh = np.uint64(32)
    idx = np.arange(n, dtype=np.uint64)
    c = [idx & mask, idx >> sh, np.full(n, offset & 0xFFFFFFFF, dtype=np.uint64),
         np.full(n, offset >> 32, dtype=np.uint64)]
    k0, k1 = np.uint64(seed & 0xFFFFFFFF), np.uint64(seed >> 32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]  # 32 x 32 -> 64 bits: no overflow
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
        k0 = (k0 + np.uint64(0x9E3779B9)) & mask
        k1 = (k1 + np.uint64(0xBB67AE85)) & mask
    return c[0]


@pytest.mark.parametrize("seed,offset", [(12345, 4), ((1 << 40) + 7919 * 3 + 1, (1 << 33) + 9)])
def test_the_draw_is_philox(cuda, seed, offset):
    from nerf_amd import ops
    got = ops.march_jitter(1000, 0.005, seed, offset, cuda)
    assert got.dtype == torch.float32 and got.shape == (1000,) and got.device.type == "cuda"
    x = _philox_first_word(1000, seed, offset)
    u = (x >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    want = u.astype(np.float32) * STEP
    assert want.dtype == np.float32
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert float(got.min()) >= 0.0 and float(got.max()) < float(STEP)
    assert len(np.unique(want)) > 990  # (a stream, not a constant)
    empty = ops.march_jitter(0, 0.005, seed, offset, cuda)
    assert empty.shape == (0,) and empty.dtype == torch.float32


# --------------------------------------------------------------------------------------
# 2. the walk stays exact under a shift
# --------------------------------------------------------------------------------------
def _axis_rays():
    """Six rays along +-x, +-y, +-z through the scene: two direction components are exactly 0."""
    rows = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            o = [0.11, -0.23, 0.37]
            d = [0.0, 0.0, 0.0]
            o[axis] = -4.0 * sign
            d[axis] = sign
            rows.append(o + d)
    return torch.tensor(rows, dtype=torch.float32)


def _checker_grid(res=128):
    """Every other cell occupied: a ray's occupied steps come in many short runs (the lego grid's rays have
    at most 13, the one-pass gather records 16 before it walks again)."""
    i = torch.arange(res)
    return (i[:, None, None] + i[None, :, None] + i[None, None, :]) % 2 == 0


def _runs(occ):
    return (occ[:, 1:] & ~occ[:, :-1]).sum(1) + occ[:, 0].long()


@pytest.fixture(scope="module")
def walk_cases(golden, lego_grid):
    """grid name -> (grid, rays, t_table, shifts, brute-force occupancy [N, 800], points [N, 800, 3])."""
    from oracle import nerf_oracle as O
    rays = torch.cat([torch.from_numpy(golden["march_rays"]), _axis_rays()])
    t = torch.from_numpy(golden["march_t_table"])
    shift = _random_shifts(rays.shape[0], 5)
    synthetic = torch.rand(33, 33, 33, generator=torch.Generator().manual_seed(9)) < 0.02
    checker = _checker_grid()
    ts = t[None, :] + shift[:, None]                               # fp32, one rounded add
    p = rays[:, None, :3] + ts[:, :, None] * rays[:, None, 3:]    # fp32, separately rounded mul and add
    assert p.dtype == torch.float32
    out = {}
    for name, grid in (("lego", lego_grid), ("synthetic", synthetic), ("checker", checker)):
        gi = O.grid_indices(p.reshape(-1, 3), res=grid.shape[0]).reshape(rays.shape[0], -1, 3)
        out[name] = (grid, rays, t, shift, grid[gi[..., 0], gi[..., 1], gi[..., 2]], p)
    return out


@pytest.mark.parametrize("use_macro", [True, False])
@pytest.mark.parametrize("name", ["lego", "synthetic", "checker"])
def test_shifted_walk_against_brute_force(cuda, walk_cases, name, use_macro):
    from nerf_amd import ops
    from nerf_amd._lib import lib, ptr, stream_of
    grid, rays, t, shift, occ, p = walk_cases[name]
    N, res = rays.shape[0], grid.shape[0]
    assert N == 262 and t.numel() == 800
    counts, runs = occ.sum(1), _runs(occ)
    print(f"\n{name}: points per ray min {int(counts.min())} max {int(counts.max())} total {int(counts.sum())}, "
          f"runs per ray max {int(runs.max())}, empty rays {int((counts == 0).sum())}")
    if name == "checker":  # not degenerate: rays of many runs here, empty and long rays on the other two
        assert int((runs > 16).sum()) > 128
    else:
        assert int((counts == 0).sum()) > 0 and int((counts > 64).sum()) > 0
    assert int(counts[256:].max()) > 0  # axis-aligned rays do cross occupied cells
    g8 = grid.to(cuda).to(torch.uint8).contiguous()
    macro = None
    if use_macro:
        macro = torch.empty(lib().nerf_march_macro_bytes(res), dtype=torch.uint8, device=cuda)
        assert lib().nerf_march_macro(ptr(g8), res, ptr(macro), stream_of(g8)) == 0
    seg_off = torch.zeros(N + 1, dtype=torch.int32, device=cuda)
    seg_off[1:] = torch.cumsum(counts.to(cuda), 0, dtype=torch.int32)
    out_ray, out_step, out_pts = (x.cpu() for x in ops.march_segments(
        rays.to(cuda), t.to(cuda), g8, macro, seg_off, int(counts.sum()), t_shift=shift.to(cuda)))
    ray_ref, step_ref = torch.nonzero(occ, as_tuple=True)
    assert torch.equal(out_ray.long(), ray_ref) and torch.equal(out_step.long(), step_ref)
    assert torch.equal(out_pts, p[ray_ref, step_ref])


# --------------------------------------------------------------------------------------
# 3. null, zeros, and groups
# --------------------------------------------------------------------------------------
def _march(f, rays, grid=None, **kw):
    from nerf_amd import ops
    kw.setdefault("t_table", f["t_table"])
    with torch.no_grad():
        return ops.march(f["net"].model_fine.packer(), rays, 2.0, 6.0, f["grid"] if grid is None else grid,
                         return_used=True, **kw)


def test_null_shift_equals_zero_shift(cuda, fixture_net):
    f = fixture_net
    a = _march(f, f["rays"])
    b = _march(f, f["rays"], t_shift=torch.zeros(256, device=cuda))
    assert a["n_queried"] == 13382 and set(a) == set(b)
    _same(a, b)


def _group_shifts(n):
    vals = torch.tensor(np.array(GROUP_SHIFTS, dtype=np.float32))
    return vals[torch.arange(n) % 4]


def test_groups_equal_the_shifted_table(cuda, fixture_net):
    f = fixture_net
    shift = _group_shifts(256).to(cuda)
    out = _march(f, f["rays"], t_shift=shift)
    total = 0
    for g, c in enumerate(GROUP_SHIFTS):
        idx = torch.arange(g, 256, 4, device=cuda)
        table_c = f["t_table"] + torch.tensor(c, dtype=torch.float32, device=cuda)
        assert table_c.dtype == torch.float32
        ref = _march(f, f["rays"][idx].contiguous(), t_table=table_c)
        for k in MAPS + ("ray_used",):
            assert torch.equal(out[k][idx], ref[k]), (k, float(c))
        total += ref["n_queried"]
    assert total == out["n_queried"] == int(out["ray_used"].sum()) > 0
    plain = _march(f, f["rays"])  # (the shift does move the result: the test would show nothing otherwise)
    assert not torch.equal(plain["depth_map_f"], out["depth_map_f"])
    assert torch.equal(plain["depth_map_f"][::4], out["depth_map_f"][::4])  # ... except the group of shift 0


def test_groups_equal_the_shifted_table_with_many_runs(cuda, fixture_net):
    """The same on a grid whose rays have more runs of occupied steps than the one-pass gather records (16):
    K = 768 from the first round, so a ray's gather overflows its run slots and walks again, shifted."""
    f = fixture_net
    grid = _checker_grid().to(cuda)
    shift = _group_shifts(256).to(cuda)
    kw = dict(grid=grid, k_schedule=(768,))
    out = _march(f, f["rays"], t_shift=shift, **kw)
    # a cell's chord is at most sqrt(3) * 3 / 127 = 0.041 = 8.2 steps: more than 16 * 9 points are more than 16 runs
    assert int(out["ray_used"].max()) > 144
    for g, c in enumerate(GROUP_SHIFTS):
        idx = torch.arange(g, 256, 4, device=cuda)
        ref = _march(f, f["rays"][idx].contiguous(),
                     t_table=f["t_table"] + torch.tensor(c, dtype=torch.float32, device=cuda), **kw)
        for k in MAPS + ("ray_used",):
            assert torch.equal(out[k][idx], ref[k]), (k, float(c))
    # the two-pass form (gather, then emit walking again) reads the same shifts
    two = _march(f, f["rays"], t_shift=shift, one_pass=False, **kw)
    _same(out, two, MAPS + ("ray_used", "n_queried"))


SEG_LENGTHS = [0, 1, 63, 64, 65, 129, 800]
ALPHA_ONE = (6, 300)   # (segment, position): raw[3] = 1e4 -> alpha is exactly 1
SURPLUS = {5: 4}       # segment -> length of its -1 tail


def _segment_case(shift_of):
    g = torch.Generator().manual_seed(4)
    N = 24
    lens = SEG_LENGTHS + torch.randint(0, 201, (N - len(SEG_LENGTHS),), generator=g).tolist()
    steps = []
    for i, n in enumerate(lens):
        s = torch.randperm(800, generator=g)[:n].sort().values.to(torch.int32)
        if i in SURPLUS:
            s[n - SURPLUS[i]:] = -1
        steps.append(s)
    seg_off = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    M = int(seg_off[-1])
    raw = torch.randn(M, 4, generator=g)
    raw[:, :3] *= 2.0
    raw[:, 3] *= 40.0
    raw[int(seg_off[ALPHA_ONE[0]]) + ALPHA_ONE[1], 3] = 1e4
    rays = torch.cat([torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)], 1)
    cot = (torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g))
    return dict(N=N, lens=lens, seg_off=seg_off, out_step=torch.cat(steps), raw=raw, rays=rays, cot=cot,
                t_table=torch.arange(2.0, 6.0, 0.005), shift=shift_of(N))


def _seg_run(c, cuda, white, t_table, t_shift):
    from nerf_amd import ops
    raw = c["raw"].to(cuda).requires_grad_(True)
    args = (raw, c["rays"].to(cuda), t_table.to(cuda), c["seg_off"].to(cuda), c["out_step"].to(cuda), 0.005, white)
    if t_shift is not None:
        args += (t_shift.to(cuda),)
    rgb, depth, acc = ops._MarchSegComposite.apply(*args)
    (g_raw,) = torch.autograd.grad([rgb, depth, acc], [raw], [x.to(cuda) for x in c["cot"]])
    return rgb.detach().cpu(), depth.detach().cpu(), acc.detach().cpu(), g_raw.cpu()


@pytest.mark.parametrize("white", [False, True])
def test_segment_groups_equal_the_shifted_table(cuda, white):
    c = _segment_case(_group_shifts)
    assert c["t_table"].numel() == 800
    got = _seg_run(c, cuda, white, c["t_table"], c["shift"])
    off = c["seg_off"].tolist()
    for g, val in enumerate(GROUP_SHIFTS):
        ref = _seg_run(c, cuda, white, c["t_table"] + torch.tensor(val, dtype=torch.float32), None)
        rows = list(range(g, c["N"], 4))
        for a, b, what in zip(got[:3], ref[:3], ("rgb", "depth", "acc")):
            assert torch.equal(a[rows], b[rows]), (what, float(val))
        for r in rows:
            assert torch.equal(got[3][off[r]:off[r + 1]], ref[3][off[r]:off[r + 1]]), (r, float(val))
    plain = _seg_run(c, cuda, white, c["t_table"], None)
    assert not torch.equal(plain[1], got[1]) and not torch.equal(plain[3], got[3])  # (the shift reaches both)


# --------------------------------------------------------------------------------------
# 4. the segment kernels with a shift against fp64
# --------------------------------------------------------------------------------------
def _segment_reference(c, white, step_size=0.005):
    """fp64, out of place: sigmoid / relu, alpha, exclusive cumprod, weighted sums, per ray; the depth of
    a point is float64(float32(t_table[s] + shift[r]))."""
    raw = c["raw"].double().requires_grad_(True)
    off = c["seg_off"].tolist()
    rgb, depth, acc = [], [], []
    for r in range(c["N"]):
        sl = slice(off[r], off[r + 1])
        st = c["out_step"][sl].long()
        valid = (st >= 0).double()
        col = torch.sigmoid(raw[sl, :3])
        sigma = torch.relu(raw[sl, 3])
        dist = step_size * torch.linalg.vector_norm(c["rays"][r, 3:6].double())
        alpha = (1.0 - torch.exp(-sigma * dist)) * valid
        T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(1.0 - alpha, 0)[:-1]])
        w = T * alpha
        t32 = c["t_table"][st.clamp(min=0)] + c["shift"][r]
        assert t32.dtype == torch.float32
        t = t32.double()
        a = w.sum()
        rgb.append((w[:, None] * col).sum(0) + ((1.0 - a) if white else 0.0))
        depth.append((w * t).sum())
        acc.append(a)
    rgb, depth, acc = torch.stack(rgb), torch.stack(depth), torch.stack(acc)
    g_rgb, g_depth, g_acc = (x.double() for x in c["cot"])
    (g_raw,) = torch.autograd.grad((rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum(), raw)
    return rgb.detach(), depth.detach(), acc.detach(), g_raw


@pytest.mark.parametrize("white", [False, True])
def test_shifted_segment_kernels_against_fp64(cuda, white):
    c = _segment_case(lambda n: _random_shifts(n, 6))
    rgb, depth, acc, g = _seg_run(c, cuda, white, c["t_table"], c["shift"])
    r_rgb, r_depth, r_acc, r_graw = _segment_reference(c, white)
    np.testing.assert_allclose(rgb.numpy(), r_rgb.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(acc.numpy(), r_acc.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(depth.numpy(), r_depth.numpy(), rtol=0, atol=5e-5)
    assert rgb[0].tolist() == [1.0 if white else 0.0] * 3 and float(depth[0]) == 0.0 and float(acc[0]) == 0.0
    assert bool(torch.isfinite(g).all())
    print(f"\nwhite {white}: g_raw max abs err {float((g.double() - r_graw).abs().max()):.3e} "
          f"(largest entry {float(r_graw.abs().max()):.3e})")
    np.testing.assert_allclose(g.numpy(), r_graw.numpy(), rtol=1e-4, atol=1e-5)
    off = c["seg_off"].tolist()
    seg, pos = ALPHA_ONE
    tail = g[off[seg] + pos + 1:off[seg + 1]]
    assert tail.numel() > 0 and bool((tail == 0).all())
    assert bool((g[c["out_step"] < 0] == 0).all())


# --------------------------------------------------------------------------------------
# 5. the gradient end to end
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
def test_gradient_with_one_shift_equals_the_shifted_table(cuda, fixture_net, dtype):
    f = fixture_net
    c = torch.tensor(0.00125, dtype=torch.float32, device=cuda)
    shifted = _march_grad(f, f["rays"], dtype, t_shift=torch.full((256,), 0.00125, device=cuda))
    g_shifted = _flat_grad(f, _loss(shifted, f["gt"]))
    table = _march_grad(f, f["rays"], dtype, t_table=f["t_table"] + c)
    g_table = _flat_grad(f, _loss(table, f["gt"]))
    assert shifted["n_queried"] == table["n_queried"] > 0
    for m in MAPS:
        assert torch.equal(shifted[m].detach(), table[m].detach()), m
    assert float(g_table.abs().max()) > 0 and torch.equal(g_shifted, g_table)
    g_plain = _flat_grad(f, _loss(_march_grad(f, f["rays"], dtype), f["gt"]))
    assert not torch.equal(g_plain, g_shifted)  # (the shift does reach the gradient)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
def test_gradient_with_per_ray_shifts_is_reproducible(cuda, fixture_net, dtype):
    f = fixture_net
    shift = _random_shifts(256, 7).to(cuda)
    flats, outs = [], []
    for _ in range(2):
        out = _march_grad(f, f["rays"], dtype, t_shift=shift)
        flats.append(_flat_grad(f, _loss(out, f["gt"])))
        outs.append(out)
    assert float(flats[0].abs().max()) > 0 and torch.equal(flats[0], flats[1])
    nograd = _march(f, f["rays"], t_shift=shift, dtype=dtype)
    assert outs[0]["n_queried"] == nograd["n_queried"]
    for m in MAPS:
        assert outs[0][m].requires_grad, m
        diff = float((outs[0][m].detach() - nograd[m]).abs().max())
        print(f"\n{dtype} {m}: differentiable forward against the no-grad march, max abs diff {diff:.3e}")
        np.testing.assert_allclose(outs[0][m].detach().cpu().numpy(), nograd[m].cpu().numpy(), rtol=0, atol=1e-4,
                                   err_msg=m)


# --------------------------------------------------------------------------------------
# 6. under a point budget
# --------------------------------------------------------------------------------------
def test_budget_cuts_the_shift_with_the_rays(cuda, fixture_net):
    f = fixture_net
    B = 6000
    shift = _random_shifts(256, 8).to(cuda)
    capped = _march_grad(f, f["rays"], "fp32", t_shift=shift, max_points=B)
    kept = capped["rays_kept"]
    assert 0 < kept < 256 and capped["n_points"] <= B
    g_capped = _flat_grad(f, _loss(capped, f["gt"], kept))
    alone = _march_grad(f, f["rays"][:kept], "fp32", t_shift=shift[:kept])
    g_alone = _flat_grad(f, _loss(alone, f["gt"][:kept]))
    assert alone["n_queried"] == capped["n_points"]
    for m in MAPS:
        assert capped[m].shape[0] == 256 and torch.equal(capped[m][:kept].detach(), alone[m].detach()), m
    assert float(g_alone.abs().max()) > 0 and torch.equal(g_capped, g_alone)
    nograd = _march(f, f["rays"], t_shift=shift)  # pass A
    assert nograd["n_queried"] == capped["n_queried"]
    for m in MAPS:
        assert torch.equal(capped[m][kept:].detach(), nograd[m][kept:]), m
    # an unshifted budgeted call keeps another prefix or other rows: the shift took part in pass A
    plain = _march_grad(f, f["rays"], "fp32", max_points=B)
    assert not torch.equal(plain["depth_map_f"].detach(), capped["depth_map_f"].detach())


# --------------------------------------------------------------------------------------
# 7. the trainer
# --------------------------------------------------------------------------------------
def test_trainer_with_jitter(cuda, jcfg, g2, trained_grid, tmp_path, monkeypatch):
    cfg = jcfg
    ta = cfg.task_arg
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.train_march_jitter = True
    step = np.float32(ta.render_step_size)
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt)
    runs = []
    for _ in range(2):
        net, trainer, opt = _trainer(cfg, cuda)
        assert trainer.network.march_jitter is True
        shifts = []
        for _ in range(2):
            out, loss, stats = trainer.train_step(dict(batch), opt)
            assert set(stats) == {"loss_f", "total_loss"} and bool(torch.isfinite(loss))
            s = out["t_shift"]
            assert s.dtype == torch.float32 and s.shape == (256,)
            assert float(s.min()) >= 0.0 and float(s.max()) < float(step)
            shifts.append(s.clone())
        assert not torch.equal(shifts[0], shifts[1])
        assert trainer.network.renderer._calls == 2
        torch.cuda.synchronize()
        runs.append((shifts, [p.detach().clone() for p in net.parameters()]))
    for a, b in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    # validation keeps render(): no march, no jitter
    with torch.no_grad():
        ret, _, _ = trainer.network(dict(batch))
    assert "rgb_map_c" in ret and "t_shift" not in ret


def test_chunked_jittered_step_equals_unchunked(cuda, jcfg, g2, trained_grid):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg = jcfg
    cfg.task_arg.train_march_jitter = True
    net = _trained_net(cuda)
    rays = np.concatenate([g2["march_rays"], g2["march_rays"][:44][::-1]])  # 300 rays
    outs = []
    for chunk in (4096, 128):  # one chunk, then three; two renderers of the same seed at the same call count
        cfg.task_arg.chunk_size = chunk
        r = Renderer(net)
        r.set_occupancy_grid(trained_grid, cuda)
        outs.append(r.render_accelerated(_batch(rays, cuda)))
        assert r._calls == 1
    whole, parts = outs
    assert parts["n_queried"] == whole["n_queried"]
    assert whole["t_shift"].shape == (300,) and torch.equal(parts["t_shift"], whole["t_shift"])
    for m in MAPS:
        assert parts[m].shape[0] == 300 and torch.equal(parts[m], whole[m]), m
    # the two copies of a ray drew different shifts (one draw over the batch, not one per chunk of rays)
    assert not torch.equal(whole["t_shift"][:44], whole["t_shift"][256:].flip(0))


def test_key_off_draws_nothing_and_no_grad_never_jitters(cuda, jcfg, g2, trained_grid, tmp_path, monkeypatch):
    from nerf_amd import ops
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg = jcfg
    ta = cfg.task_arg
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.train_march_jitter = False
    gt = torch.rand(256, 3, generator=torch.Generator().manual_seed(1))
    batch = _batch(g2["march_rays"], cuda, gt)
    net, trainer, opt = _trainer(cfg, cuda)
    calls = trainer.network.renderer._calls
    out, _, _ = trainer.train_step(dict(batch), opt)
    assert "t_shift" not in out and trainer.network.renderer._calls == calls
    # without grad, whatever the key says: the unjittered march, nothing drawn
    ta.train_march_jitter = True
    net = _trained_net(cuda)
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    with torch.no_grad():
        inf = r.render_accelerated(_batch(g2["march_rays"], cuda))
        ref = ops.march(net.model_fine.packer(), torch.from_numpy(g2["march_rays"]).to(cuda), 2.0, 6.0,
                        r.occupancy_grid, step_size=float(ta.render_step_size),
                        t_thresh=float(ta.transmittance_threshold), bbox=r._bbox_tuple(),
                        white_bkgd=bool(ta.white_bkgd), dtype=net.mlp_dtype)
    assert "t_shift" not in inf and r._calls == 0 and inf["n_queried"] == ref["n_queried"]
    for m in MAPS:
        assert torch.equal(inf[m], ref[m]), m


# --------------------------------------------------------------------------------------
# 8. it trains
# --------------------------------------------------------------------------------------
def test_it_trains_with_jitter(cuda, jcfg, g2, trained_grid, tmp_path, monkeypatch):
    """test_it_trains with the key on: rgb_linear.bias + 1, gt = the unperturbed net's unjittered march, 12
    steps (lr 5e-4, clip 40).  The target is smooth along the ray at this net, so sub-step jitter moves the
    loss little: the unjittered first loss is 0.0285161."""
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg = jcfg
    ta = cfg.task_arg
    _write_grid(tmp_path, monkeypatch, trained_grid)
    ta.train_renderer = "accelerated"
    ta.train_grid = "file"
    ta.train_march_jitter = True
    assert float(cfg.train.lr) == 5e-4
    net = _trained_net(cuda)
    with torch.no_grad():
        net.model_fine.rgb_linear.bias += 1.0
    trainer = make_trainer(cfg, net)
    assert trainer.clip_value == 40.0
    opt = make_optimizer(cfg, net)
    batch = _batch(g2["march_rays"], cuda, g2["march_rgb_map_f"])
    losses = []
    for _ in range(12):
        out, loss, _ = trainer.train_step(dict(batch), opt)
        assert "t_shift" in out
        losses.append(float(loss))
    print("\nlosses:", " ".join(f"{v:.6f}" for v in losses), f"(first, unjittered: 0.0285161; ratio "
          f"{losses[0] / 0.0285161:.4f})")
    assert losses[11] < 0.25 * losses[0], losses
