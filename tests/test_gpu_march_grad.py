"""The differentiable grid march on the GPU: render_accelerated under autograd.

Pass A (ops.march, no grad) decides which points each ray composites; pass B lays them out
contiguously in ray order (nerf_march_segments), runs the training MLP once with a per-sample
direction index, and composites every segment with a differentiable kernel pair
(nerf_march_seg_composite_fwd / _bwd).  Checked here:

  * the segment kernels against an fp64 out-of-place restatement (alpha == 1, surplus points,
    chunk boundaries, empty segments);
  * the per-count gather against a brute-force occupancy test of every step;
  * ray_used: its sum is n_queried, the other outputs unchanged bit for bit;
  * the MLP with dir_index under autograd == the MLP with the directions expanded;
  * the differentiable forward == the march fixtures of golden_v1 / golden_v2;
  * the gradients against the reference's (tests/golden/golden_march_grad.npz), four tiers;
  * bit-reproducibility through the flat-gradient path; edge cases; one Trainer.train_step
    with task_arg.train_renderer "accelerated" against autograd + clip + torch Adam; 12 steps
    of it bring a perturbed net back.
"""
import os

import numpy as np
import pytest
import torch

from march_support import MAPS, _batch, _write_grid, g2, lego_grid, mg, trained_grid

pytestmark = pytest.mark.gpu

os.environ.setdefault("NERF_AMD_NO_ARGV", "1")
HERE = os.path.dirname(os.path.abspath(__file__))


def _net(state, cuda):
    from src.config import cfg
    from src.models.nerf.network import Network
    cfg.task_arg.perturb = 0
    cfg.task_arg.mlp_dtype = "fp32"
    torch.manual_seed(0)
    net = Network()
    net.load_state_dict(state, strict=True)
    return net.to(cuda)


@pytest.fixture()
def trained(cuda):
    """A fresh trained-fixture net per test (tests here step and perturb it)."""
    from src.config import cfg
    z = np.load(os.path.join(HERE, "golden", "trained_v2.npz"), allow_pickle=False)
    net = _net({k: torch.from_numpy(z[k]) for k in z.files}, cuda)
    yield cfg, net
    cfg.task_arg.mlp_dtype = "fp32"
    cfg.task_arg.train_renderer = "hierarchical"
    cfg.task_arg.chunk_size = 4096


@pytest.fixture()
def seeded(cuda, seeded_state):
    from src.config import cfg
    return cfg, _net(seeded_state, cuda)


# --------------------------------------------------------------------------------------
# 1. the segment compositing kernels against an fp64 restatement
# --------------------------------------------------------------------------------------
SEG_LENGTHS = [0, 1, 2, 63, 64, 65, 128, 129, 509, 800]
ALPHA_ONE = [(8, 200), (9, 400), (7, 64)]  # (segment, position): raw[3] = 1e4 -> alpha is exactly 1
SURPLUS = {6: 1, 7: 5}                      # segment -> length of its -1 tail


def _segment_case():
    g = torch.Generator().manual_seed(3)
    N = 67
    lens = SEG_LENGTHS + torch.randint(0, 201, (N - len(SEG_LENGTHS),), generator=g).tolist()
    steps = []
    for i, n in enumerate(lens):
        s = torch.randperm(800, generator=g)[:n].sort().values.to(torch.int32)  # strictly increasing
        if i in SURPLUS:
            s[n - SURPLUS[i]:] = -1
        steps.append(s)
    seg_off = torch.tensor([0] + np.cumsum(lens).tolist(), dtype=torch.int32)
    M = int(seg_off[-1])
    raw = torch.randn(M, 4, generator=g)
    raw[:, :3] *= 2.0   # rgb logits ~ N(0, 2)
    raw[:, 3] *= 40.0   # about half <= 0; sigma * dist ~ 0.2 |d|: the transmittance decays within a segment
    for seg, pos in ALPHA_ONE:
        raw[int(seg_off[seg]) + pos, 3] = 1e4
    rays = torch.cat([torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g)], 1)
    cot = (torch.randn(N, 3, generator=g), torch.randn(N, generator=g), torch.randn(N, generator=g))
    return dict(N=N, lens=lens, seg_off=seg_off, out_step=torch.cat(steps), raw=raw, rays=rays, cot=cot,
                t_table=torch.arange(2.0, 6.0, 0.005))


def _segment_reference(c, white, step_size=0.005):
    """fp64, out of place: sigmoid / relu, alpha, exclusive cumprod, weighted sums, per ray."""
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
        t = c["t_table"][st.clamp(min=0)].double()
        a = w.sum()
        rgb.append((w[:, None] * col).sum(0) + ((1.0 - a) if white else 0.0))
        depth.append((w * t).sum())
        acc.append(a)
    rgb, depth, acc = torch.stack(rgb), torch.stack(depth), torch.stack(acc)
    g_rgb, g_depth, g_acc = (x.double() for x in c["cot"])
    (g_raw,) = torch.autograd.grad((rgb * g_rgb).sum() + (depth * g_depth).sum() + (acc * g_acc).sum(), raw)
    return rgb.detach(), depth.detach(), acc.detach(), g_raw


@pytest.fixture(scope="module")
def segment_case():
    c = _segment_case()
    c["ref"] = {white: _segment_reference(c, white) for white in (False, True)}  # computed once, shared
    return c


@pytest.mark.parametrize("white", [False, True])
def test_segment_kernels_against_fp64(cuda, segment_case, white):
    from nerf_amd import ops
    c = segment_case
    raw = c["raw"].to(cuda).requires_grad_(True)
    rgb, depth, acc = ops._MarchSegComposite.apply(raw, c["rays"].to(cuda), c["t_table"].to(cuda),
                                                   c["seg_off"].to(cuda), c["out_step"].to(cuda), 0.005, white)
    (g_raw,) = torch.autograd.grad([rgb, depth, acc], [raw], [x.to(cuda) for x in c["cot"]])
    r_rgb, r_depth, r_acc, r_graw = c["ref"][white]
    # forward: the bounds of test_render_accelerated_real_grid
    np.testing.assert_allclose(rgb.detach().cpu().numpy(), r_rgb.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(acc.detach().cpu().numpy(), r_acc.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(depth.detach().cpu().numpy(), r_depth.numpy(), rtol=0, atol=5e-5)
    # empty segments: background / zero
    empty = [i for i, n in enumerate(c["lens"]) if n == 0]
    assert 0 in empty
    for i in empty:
        assert rgb[i].tolist() == [1.0 if white else 0.0] * 3 and float(depth[i]) == 0.0 and float(acc[i]) == 0.0
    g = g_raw.cpu()
    assert bool(torch.isfinite(g).all())
    print(f"\nwhite {white}: g_raw max abs err {float((g.double() - r_graw).abs().max()):.3e} "
          f"(largest entry {float(r_graw.abs().max()):.3e})")
    # backward: the bounds of test_composite_backward
    np.testing.assert_allclose(g.numpy(), r_graw.numpy(), rtol=1e-4, atol=1e-5)
    off = c["seg_off"].tolist()
    for seg, pos in ALPHA_ONE:  # T is exactly 0 after an alpha == 1 point
        tail = g[off[seg] + pos + 1:off[seg + 1]]
        assert tail.numel() > 0 and bool((tail == 0).all()), seg
    for seg, n in SURPLUS.items():
        assert bool((g[off[seg + 1] - n:off[seg + 1]] == 0).all()), seg
    assert bool((g[c["out_step"] < 0] == 0).all())


# --------------------------------------------------------------------------------------
# 2. the per-count gather against brute force
# --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def brute(golden, lego_grid):
    """Occupancy of every step of golden_v1's 256 march rays on the lego grid (CPU, the
    reference's index arithmetic): [256, 800] bool and the points."""
    from oracle import nerf_oracle as O
    rays = torch.from_numpy(golden["march_rays"])
    t = torch.from_numpy(golden["march_t_table"])
    p = rays[:, None, :3] + t[None, :, None] * rays[:, None, 3:]
    gi = O.grid_indices(p.reshape(-1, 3), res=lego_grid.shape[0]).reshape(rays.shape[0], -1, 3)
    return lego_grid[gi[..., 0], gi[..., 1], gi[..., 2]], p


@pytest.mark.parametrize("use_macro", [True, False])
def test_march_segments_against_brute_force(golden, cuda, lego_grid, brute, use_macro):
    from nerf_amd import ops
    from nerf_amd._lib import lib, ptr, stream_of
    occ, p = brute
    counts = occ.sum(1)
    assert (int(counts.min()), float(counts.float().median()), int(counts.max())) == (0, 197.0, 509)
    assert int((counts == 0).sum()) == 72 and int(counts.sum()) == 44974
    rays = torch.from_numpy(golden["march_rays"]).to(cuda)
    t = torch.from_numpy(golden["march_t_table"]).to(cuda)
    g8 = lego_grid.to(cuda).to(torch.uint8).contiguous()
    macro = None
    if use_macro:
        macro = torch.empty(lib().nerf_march_macro_bytes(128), dtype=torch.uint8, device=cuda)
        assert lib().nerf_march_macro(ptr(g8), 128, ptr(macro), stream_of(g8)) == 0
    ray_ref, step_ref = torch.nonzero(occ, as_tuple=True)

    def run(cnt):
        seg_off = torch.zeros(257, dtype=torch.int32, device=cuda)
        seg_off[1:] = torch.cumsum(cnt.to(cuda), 0, dtype=torch.int32)
        return ops.march_segments(rays, t, g8, macro, seg_off, int(cnt.sum()))

    out_ray, out_step, out_pts = (x.cpu() for x in run(counts))
    assert torch.equal(out_ray.long(), ray_ref) and torch.equal(out_step.long(), step_ref)
    assert torch.equal(out_pts, p[ray_ref, step_ref])
    # counts + 3 on four rays (an empty one, the longest, two others): the surplus is -1 / the ray / its origin
    more = counts.clone()
    bumped = [int((counts == 0).nonzero()[0]), int(counts.argmax()), 5, 255]
    more[bumped] += 3
    out_ray, out_step, out_pts = (x.cpu() for x in run(more))
    off = [0] + torch.cumsum(more, 0).tolist()
    for r in range(256):
        n = int(counts[r])
        sl = slice(off[r], off[r] + n)
        assert torch.equal(out_step[sl].long(), step_ref[ray_ref == r]), r
        assert bool((out_ray[off[r]:off[r + 1]] == r).all()), r
        if r in bumped:
            tail = slice(off[r] + n, off[r + 1])
            assert off[r + 1] - off[r] - n == 3
            assert bool((out_step[tail] == -1).all()) and torch.equal(out_pts[tail], rays[r, :3].cpu().expand(3, 3))


# --------------------------------------------------------------------------------------
# 3. ray_used
# --------------------------------------------------------------------------------------
def _march_case(tag, golden, g2, lego_grid, trained_grid):
    if tag == "trained":
        return g2["march_rays"], trained_grid, int(g2["march_queried"]), {k: g2[f"march_{k}"] for k in MAPS}
    return (golden["march_rays"], lego_grid, int(golden[f"march_{tag}_queried"]),
            {k: golden[f"march_{tag}_{k}"] for k in MAPS})


def _net_for(tag, request):
    cfg, net = request.getfixturevalue("trained" if tag == "trained" else "seeded")
    if tag == "dense":
        with torch.no_grad():
            net.model_fine.alpha_linear.bias += 50.0
    return cfg, net


@pytest.mark.parametrize("tag,total", [("sparse", 44974), ("dense", 6481), ("trained", 13382)])
def test_ray_used(request, golden, g2, cuda, lego_grid, trained_grid, tag, total):
    from nerf_amd import ops
    rays, grid, queried, _ = _march_case(tag, golden, g2, lego_grid, trained_grid)
    assert queried == total
    _, net = _net_for(tag, request)
    rays, grid = torch.from_numpy(rays).to(cuda), grid.to(cuda)
    p = net.model_fine.packer()
    with torch.no_grad():
        a = ops.march(p, rays, 2.0, 6.0, grid)
        b = ops.march(p, rays, 2.0, 6.0, grid, return_used=True)
    assert "ray_used" not in a
    used = b["ray_used"]
    assert used.dtype == torch.int32 and used.shape == (rays.shape[0],)
    assert int(used.sum()) == b["n_queried"] == a["n_queried"] == total
    assert set(b) - set(a) == {"ray_used"}
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k


# --------------------------------------------------------------------------------------
# 4. the MLP with a per-sample direction index under autograd
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
def test_mlp_dir_index_autograd(cuda, seeded_state, dtype):
    from nerf_amd import ops
    g = torch.Generator().manual_seed(11)
    M, D = 1000, 37
    pts = (torch.rand(M, 3, generator=g) * 2.6 - 1.3).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(D, 3, generator=g), dim=-1).to(cuda)
    idx = torch.randint(0, D, (M,), generator=g).to(torch.int32).to(cuda)
    cot = torch.randn(M, 4, generator=g).to(cuda)
    params = [seeded_state[f"model_fine.{n}"].to(cuda).clone().requires_grad_(True) for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    raw_i = ops.mlp(packer, pts, vd, 1, idx, dtype)
    g_i = torch.autograd.grad(raw_i, params, cot)
    raw_e = ops.mlp(packer, pts, vd[idx.long()].contiguous(), 1, None, dtype)
    g_e = torch.autograd.grad(raw_e, params, cot)
    assert torch.equal(raw_i, raw_e)
    assert len(g_i) == 24
    for n, a, b in zip(ops.NET_PARAM_NAMES, g_i, g_e):
        assert torch.equal(a, b) and float(a.abs().max()) > 0, n


# --------------------------------------------------------------------------------------
# 5. the differentiable forward equals the march
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["sparse", "dense", "trained"])
def test_forward_equals_the_march(request, golden, g2, cuda, lego_grid, trained_grid, tag):
    from src.models.nerf.renderer.volume_renderer import Renderer
    rays, grid, queried, maps = _march_case(tag, golden, g2, lego_grid, trained_grid)
    _, net = _net_for(tag, request)
    r = Renderer(net)
    r.set_occupancy_grid(grid, cuda)
    assert torch.is_grad_enabled()
    out = r.render_accelerated(_batch(rays, cuda))
    assert out["n_queried"] == queried
    assert {"render_time", "n_queried", "n_evaluated", "rounds"} <= set(out)
    for k in MAPS:
        assert out[k].requires_grad, k
        # the bounds of the fixtures' own tests (test_gpu_render.py / test_gpu_trained.py)
        atol = 1e-4 if tag == "trained" else (5e-5 if "depth" in k else 1e-5)
        np.testing.assert_allclose(out[k].detach().cpu().numpy(), maps[k], rtol=0, atol=atol, err_msg=k)
    with torch.no_grad():  # and without grad: today's path, detached
        inf = r.render_accelerated(_batch(rays, cuda))
    assert not inf["rgb_map_f"].requires_grad and inf["n_queried"] == queried


# --------------------------------------------------------------------------------------
# 6. gradients against the reference
# --------------------------------------------------------------------------------------
def _grad_check(net, gold, tag, rel):
    """The criterion of test_gpu_trained.py::_grad_check, restated: every sampled entry within rel x its
    tensor's largest (or 1e-8), every tensor norm within rel; returns (worst entry error, relative L2)."""
    params = dict(net.named_parameters())
    worst, worst_norm = (0.0, ""), (-1.0, "")
    num = den = 0.0
    fails = []
    for i, name in enumerate(gold[f"{tag}_names"]):
        g = params[str(name)].grad.reshape(-1).double().cpu()
        norm = float(torch.linalg.vector_norm(g))
        ref_norm = float(gold[f"{tag}_norms"][i])
        if abs(norm - ref_norm) > 1e-8 + rel * abs(ref_norm):
            fails.append((str(name), "norm", norm, ref_norm))
        worst_norm = max(worst_norm, (abs(norm - ref_norm) / ref_norm, str(name)))
        sel = g[torch.from_numpy(gold[f"{tag}_sel_idx"][i])].numpy()
        scale = float(gold[f"{tag}_absmax"][i]) + 1e-30
        err = float(np.abs(sel - gold[f"{tag}_sel_val"][i]).max())
        num += float((((sel - gold[f"{tag}_sel_val"][i]) / scale) ** 2).sum())
        den += float(((gold[f"{tag}_sel_val"][i] / scale) ** 2).sum())
        if err >= 1e-8:
            worst = max(worst, (err / scale, str(name)))
    l2 = float(np.sqrt(num / den))
    print(f"\n{tag}: largest entry error {worst[0]:.2e} of the tensor's largest ({worst[1]}), "
          f"norm {worst_norm[0]:.2e} ({worst_norm[1]}), sampled-entry relative L2 {l2:.2e}")
    assert not fails, fails
    assert worst[0] < rel, worst
    return worst[0], l2


def _mg_loss(out, gt, tag):
    mse = torch.nn.functional.mse_loss(out["rgb_map_f"], gt)
    return mse if tag == "mg_rgb" else mse + 0.1 * out["depth_map_f"].mean() + 0.1 * out["acc_map_f"].mean()


# fp32: the project's fp32 contract.  The other tiers: 2x the worst error (sampled entry against its tensor's largest,
# or tensor norm) measured on the MI355X against this fixture, the measured value beside each bound.  bf16x3 is above
# the 2e-3 its hierarchical gradients hold (test_gpu_trained.py GRAD_REL; the worst entries are in
# pts_linears.0.weight, the norms are 40x closer); bf16x3f stays under its 6e-3 there.
MG_REL = {
    "fp32": {"mg_rgb": 1e-4, "mg_all": 1e-4},          # measured 6.17e-06 / 7.64e-06
    "bf16x3": {"mg_rgb": 4.4e-3, "mg_all": 6.4e-3},    # measured 2.19e-03 / 3.16e-03 (norms 3.07e-05 / 5.18e-05)
    "bf16x3f": {"mg_rgb": 4.5e-3, "mg_all": 6.5e-3},   # measured 2.23e-03 / 3.23e-03 (norms 8.14e-04 / 9.52e-04)
    "bf16": {"mg_rgb": 8.7e-2, "mg_all": 1.11e-1},     # measured 4.33e-02 / 5.53e-02 (13,386 points queried)
}


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16x3f", "bf16"])
@pytest.mark.parametrize("tag", ["mg_rgb", "mg_all"])
def test_gradients_against_reference(g2, mg, cuda, trained, trained_grid, tag, dtype):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg, net = trained
    net.mlp_dtype = dtype
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    net.zero_grad()
    out = r.render_accelerated(_batch(g2["march_rays"], cuda))
    if dtype == "fp32":
        assert out["n_queried"] == 13382 == int(mg[f"{tag}_queried"])  # (precondition of the fp32 bound)
    loss = _mg_loss(out, torch.from_numpy(mg["gt"]).to(cuda), tag)
    loss.backward()
    print(f"\n{dtype} {tag}: loss {float(loss):.8f} (reference {float(mg[f'{tag}_loss']):.8f}), "
          f"queried {out['n_queried']}")
    if dtype == "fp32":
        np.testing.assert_allclose(float(loss), float(mg[f"{tag}_loss"]), rtol=1e-5)
    for name, p in net.named_parameters():  # the coarse net is not part of the graph
        if name.startswith("model."):
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
    _grad_check(net, mg, tag, MG_REL[dtype][tag])
    net.zero_grad()


# --------------------------------------------------------------------------------------
# 7. bit-reproducible through the flat-gradient path
# --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16x3f"])
def test_flat_gradient_is_bit_reproducible(g2, mg, cuda, trained, trained_grid, dtype):
    from nerf_amd import ops
    from src.models.nerf.renderer.volume_renderer import Renderer
    from src.train.optimizer import make_optimizer
    cfg, net = trained
    net.mlp_dtype = dtype
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    opt = make_optimizer(cfg, net)
    gt = torch.from_numpy(mg["gt"]).to(cuda)
    flats = []
    for _ in range(2):
        opt.zero_grad()
        loss = _mg_loss(r.render_accelerated(_batch(g2["march_rays"], cuda)), gt, "mg_rgb")
        with ops.direct_grad():
            loss.backward()
        flats.append(opt.flat_grad.clone())
    assert float(flats[0].abs().max()) > 0
    assert torch.equal(flats[0], flats[1])


# --------------------------------------------------------------------------------------
# 8. edge cases
# --------------------------------------------------------------------------------------
def test_empty_grid_gives_background_and_zero_gradients(g2, cuda, trained):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg, net = trained
    r = Renderer(net)
    r.set_occupancy_grid(torch.zeros(128, 128, 128, dtype=torch.bool), cuda)
    net.zero_grad()
    out = r.render_accelerated(_batch(g2["march_rays"], cuda))
    assert out["n_queried"] == 0
    assert bool((out["rgb_map_f"] == 1.0).all()) and bool((out["depth_map_f"] == 0).all())
    assert bool((out["acc_map_f"] == 0).all())
    (out["rgb_map_f"].sum() + out["depth_map_f"].sum() + out["acc_map_f"].sum()).backward()
    for name, p in net.model_fine.named_parameters():
        assert p.grad is not None and float(p.grad.abs().max()) == 0.0, name


def test_one_ray_batch(g2, cuda, trained, trained_grid):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg, net = trained
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    full = r.render_accelerated(_batch(g2["march_rays"], cuda))
    k = int(full["acc_map_f"].argmax())  # a ray that hits the scene
    one = r.render_accelerated(_batch(g2["march_rays"][k:k + 1], cuda))
    assert one["n_queried"] > 0
    for m in MAPS:
        assert one[m].shape[0] == 1 and torch.equal(one[m][0], full[m][k]), m
    net.zero_grad()
    one["rgb_map_f"].sum().backward()
    assert float(net.model_fine.rgb_linear.weight.grad.abs().max()) > 0
    net.zero_grad()


def test_chunked_equals_unchunked(g2, cuda, trained, trained_grid):
    from src.models.nerf.renderer.volume_renderer import Renderer
    cfg, net = trained
    r = Renderer(net)
    r.set_occupancy_grid(trained_grid, cuda)
    rays = np.concatenate([g2["march_rays"], g2["march_rays"][:44][::-1]])  # 300 rays
    whole = r.render_accelerated(_batch(rays, cuda))
    cfg.task_arg.chunk_size = 128
    parts = r.render_accelerated(_batch(rays, cuda))
    assert parts["n_queried"] == whole["n_queried"]
    for m in MAPS:
        assert parts[m].shape[0] == 300 and torch.equal(parts[m], whole[m]), m


# --------------------------------------------------------------------------------------
# 9. the training step
# --------------------------------------------------------------------------------------
def test_training_step_accelerated(g2, mg, cuda, trained, trained_grid, tmp_path, monkeypatch):
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg, net = trained
    _write_grid(tmp_path, monkeypatch, trained_grid)
    cfg.task_arg.train_renderer = "accelerated"
    trainer = make_trainer(cfg, net)
    batch = _batch(g2["march_rays"], cuda)
    batch["rgbs"] = torch.from_numpy(mg["gt"]).to(cuda)[None]
    # the autograd path (no flat buffer yet): the loss module's own forward, a plain backward
    net.zero_grad()
    _, loss_a, stats_a = trainer.network(dict(batch))
    assert set(stats_a) == {"loss_f", "total_loss"}
    loss_a.backward()
    np.testing.assert_allclose(float(loss_a), float(mg["mg_rgb_loss"]), rtol=1e-5)
    _grad_check(net, mg, "mg_rgb", 1e-4)
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    grads = {k: (v.grad.detach().clone() if v.grad is not None else torch.zeros_like(v))
             for k, v in net.named_parameters()}
    net.zero_grad()
    opt = make_optimizer(cfg, net)  # fresh moments
    out, loss, stats = trainer.train_step(dict(batch), opt)
    torch.cuda.synchronize()
    assert set(stats) == {"loss_f", "total_loss"} and float(stats["loss_f"]) == float(stats["total_loss"])
    np.testing.assert_allclose(float(loss), float(loss_a), rtol=1e-6)
    ref = {k: v.clone().requires_grad_(True) for k, v in before.items()}
    adam = torch.optim.Adam([{"params": [p]} for p in ref.values()], lr=float(cfg.train.lr), eps=float(cfg.train.eps))
    for k, p in ref.items():
        p.grad = grads[k].clone()
    torch.nn.utils.clip_grad_value_(list(ref.values()), 40.0)
    adam.step()
    for k, p in net.named_parameters():
        np.testing.assert_allclose(p.detach().cpu().numpy(), ref[k].detach().cpu().numpy(), rtol=0, atol=1e-7,
                                   err_msg=k)
        if k.startswith("model."):  # a zero gradient and fresh moments: the coarse net does not move
            assert torch.equal(p.detach(), before[k]), k
    # validation keeps render(): without grad the loss module returns the hierarchical keys
    with torch.no_grad():
        ret, _, vstats = trainer.network(dict(batch))
    assert "rgb_map_c" in ret and "loss_c" in vstats


def test_training_needs_the_grid_file(cuda, trained, tmp_path, monkeypatch):
    from src.train.trainers.make_trainer import make_trainer
    cfg, net = trained
    monkeypatch.chdir(tmp_path)
    cfg.task_arg.train_renderer = "accelerated"
    with pytest.raises(FileNotFoundError, match="occupancy_grid.py"):
        make_trainer(cfg, net)


# --------------------------------------------------------------------------------------
# 10. it trains
# --------------------------------------------------------------------------------------
def test_it_trains(g2, cuda, trained, trained_grid, tmp_path, monkeypatch):
    """rgb_linear.bias + 1, gt = the unperturbed net's march: 12 steps (lr 5e-4, clip 40).  The
    oracle alone (CPU, autograd + torch Adam) goes 0.0285161 -> 0.00199 (0.070 x)."""
    from src.train.optimizer import make_optimizer
    from src.train.trainers.make_trainer import make_trainer
    cfg, net = trained
    _write_grid(tmp_path, monkeypatch, trained_grid)
    cfg.task_arg.train_renderer = "accelerated"
    assert float(cfg.train.lr) == 5e-4
    with torch.no_grad():
        net.model_fine.rgb_linear.bias += 1.0
    trainer = make_trainer(cfg, net)
    assert trainer.clip_value == 40.0
    opt = make_optimizer(cfg, net)
    batch = _batch(g2["march_rays"], cuda)
    batch["rgbs"] = torch.from_numpy(g2["march_rgb_map_f"]).to(cuda)[None]
    losses = []
    for _ in range(12):
        _, loss, _ = trainer.train_step(dict(batch), opt)
        losses.append(float(loss))
    print("\nlosses:", " ".join(f"{v:.6f}" for v in losses))
    np.testing.assert_allclose(losses[0], 0.0285161, rtol=1e-5)
    assert losses[11] < 0.25 * losses[0], losses
