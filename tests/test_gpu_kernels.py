"""GPU parity of each kernel family against the oracle (tests-only) and the reference goldens.

Tolerances: bit-exact for indices / masks / sample positions given identical inputs;
1e-4 absolute for fp32 rgb/depth; 2e-3 for the bf16 MLP path (north_star).
"""
import numpy as np
import pytest
import torch

from march_support import O, ops

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.asarray(x)).to(dev)


@pytest.fixture(scope="module")
def packers(seeded_state, cuda, ops):
    out = {}
    for prefix in ("model", "model_fine"):
        params = [seeded_state[f"{prefix}.{n}"].to(cuda).contiguous() for n in ops.NET_PARAM_NAMES]
        out[prefix] = ops.PackedMLP(params)
    return out


# ---------------------------------------------------------------------------------- rays
def test_raygen_matches_reference(golden, cuda, ops):
    poses = _t(golden["poses"], cuda)
    cam_x = 0.6911112070083618
    f16 = 0.5 * 16 / np.tan(0.5 * cam_x)
    pix = torch.arange(256, device=cuda)
    rays, _, _ = ops.raygen(poses[0:1], 16, 16, f16, pix=pix)
    o = golden["rays16_o"].reshape(-1, 3)
    d = golden["rays16_d"].reshape(-1, 3)
    np.testing.assert_array_equal(rays[:, :3].cpu().numpy(), o)
    np.testing.assert_allclose(rays[:, 3:].cpu().numpy(), d, rtol=0, atol=2e-7)
    f800 = 0.5 * 800 / np.tan(0.5 * cam_x)
    pix = _t(golden["pix800"], cuda) + 800 * 800  # image 1 of a 3-pose stack
    rays, _, _ = ops.raygen(poses, 800, 800, f800, pix=pix)
    np.testing.assert_array_equal(rays[:, :3].cpu().numpy(), golden["rays800_o"])
    np.testing.assert_allclose(rays[:, 3:].cpu().numpy(), golden["rays800_d"], rtol=0, atol=2e-7)


def test_raygen_random_ids_and_rgb(cuda, ops):
    poses = torch.eye(4, device=cuda).repeat(2, 1, 1)
    imgs = torch.rand(2, 8, 8, 3, device=cuda)
    rays, rgb, pix = ops.raygen(poses, 8, 8, 10.0, n_rays=4096, seed=3, images=imgs, want_pix=True)
    assert int(pix.min()) >= 0 and int(pix.max()) < 2 * 64
    assert len(torch.unique(pix)) > 100
    np.testing.assert_array_equal(rgb.cpu().numpy(), imgs.reshape(-1, 3)[pix].cpu().numpy())


def test_train_batch_reference_ids(cuda, ops):
    """a2 with the reference's own draw injected: Dataset.__getitem__ (blender.py:124-131) takes
    torch.randint(0, N_img*H*W, (n,)) over the flat ray table (blender.py:105-108: img*H*W +
    j*W + i) and gathers rays and rgb.  The same ids through nerf_raygen (pix + images): rgb
    bit-exact, o bit-exact, d within 2e-7 (the get_rays matmul's summation order)."""
    from oracle import nerf_oracle as O
    H = W = 40
    cam_x = 0.6911112070083618
    f = O.focal_from_angle(W, cam_x)
    poses = torch.stack([O.pose_spherical(float(t), -30.0, 4.0) for t in (-150.0, 10.0, 95.0)])
    imgs = torch.rand(3, H, W, 3, generator=torch.Generator().manual_seed(5))
    table_o, table_d = [], []
    for p in poses:
        o, d = O.get_rays(H, W, f, p)
        table_o.append(o.reshape(-1, 3))
        table_d.append(d.reshape(-1, 3))
    table = torch.cat([torch.cat(table_o), torch.cat(table_d)], 1)  # [N_img*H*W, 6], reference order
    torch.manual_seed(7)
    ids = torch.randint(0, table.shape[0], (4096,))                  # blender.py:126
    rays, rgb, _ = ops.raygen(poses.to(cuda), H, W, f, pix=ids.to(cuda), images=imgs.to(cuda))
    ref_rays, ref_rgb = table[ids], imgs.reshape(-1, 3)[ids]
    np.testing.assert_array_equal(rgb.cpu().numpy(), ref_rgb.numpy())
    np.testing.assert_array_equal(rays[:, :3].cpu().numpy(), ref_rays[:, :3].numpy())
    np.testing.assert_allclose(rays[:, 3:].cpu().numpy(), ref_rays[:, 3:].numpy(), rtol=0, atol=2e-7)


def test_train_batch_philox_uniform(cuda, ops):
    """The in-kernel draw replacing torch.randint is uniform over all pixels of all images:
    chi-square over 64 equal bins of the flat id, 2^20 draws (p > 1e-4), and independent
    (seed, offset) streams differ."""
    from scipy import stats
    poses = torch.eye(4, device=cuda).repeat(4, 1, 1)
    n_pix = 4 * 100 * 100
    _, _, pix = ops.raygen(poses, 100, 100, 50.0, n_rays=1 << 20, seed=11, want_pix=True)
    p = pix.cpu().numpy()
    assert p.min() >= 0 and p.max() < n_pix
    counts = np.bincount(p * 64 // n_pix, minlength=64)
    assert stats.chisquare(counts).pvalue > 1e-4, counts
    _, _, pix2 = ops.raygen(poses, 100, 100, 50.0, n_rays=1 << 20, seed=11, offset=1, want_pix=True)
    assert (pix2 != pix).float().mean().item() > 0.99


# ---------------------------------------------------------------------------------- stratified
@pytest.mark.parametrize("perturb", [False, True])
def test_stratified_bit_exact(golden, cuda, ops, O, perturb):
    rays = torch.from_numpy(golden["rays"][:64])
    t_rand = torch.from_numpy(golden["render1_t_rand"]) if perturb else None
    z_ref = O.stratified_z(64, torch.tensor([2.0]), torch.tensor([6.0]), 64, t_rand)
    pts_ref = rays[:, None, :3] + rays[:, None, 3:] * z_ref[..., None]
    z, pts, vd = ops.sample_stratified(rays.to(cuda), 2.0, 6.0, 64, perturb,
                                       t_rand.to(cuda) if perturb else None)
    np.testing.assert_array_equal(z.cpu().numpy(), z_ref.numpy())
    np.testing.assert_array_equal(pts.cpu().numpy(), pts_ref.numpy())
    vref = rays[:, 3:] / torch.norm(rays[:, 3:], dim=-1, keepdim=True)
    np.testing.assert_allclose(vd.cpu().numpy(), vref.numpy(), rtol=0, atol=2e-7)


# ---------------------------------------------------------------------------------- sample_pdf
def test_searchsorted_bit_exact(golden, cuda, ops):
    cdf = torch.from_numpy(golden["pdf_det_cdf"])
    for u in (torch.from_numpy(golden["pdf_u"]), torch.linspace(0, 1, 128).expand(64, 128).contiguous()):
        ref = torch.searchsorted(cdf, u, right=True)
        got = ops.searchsorted(cdf.to(cuda), u.to(cuda)).cpu().long()
        assert torch.equal(got, ref)
    # adversarial: u equal to cdf entries, ties, 0 and 1, duplicated cdf values
    g = torch.Generator().manual_seed(5)
    c = torch.sort(torch.rand(256, 63, generator=g), -1).values
    c[:, 0] = 0
    c[:, 20:25] = c[:, 20:21]
    uu = torch.cat([c[:, ::2], torch.rand(256, 32, generator=g), torch.zeros(256, 2), torch.ones(256, 2)], 1)
    ref = torch.searchsorted(c, uu.contiguous(), right=True)
    got = ops.searchsorted(c.to(cuda), uu.contiguous().to(cuda)).cpu().long()
    assert torch.equal(got, ref)


@pytest.mark.parametrize("det", [True, False])
def test_sample_pdf(golden, cuda, ops, O, det):
    bins = torch.from_numpy(golden["pdf_bins"])
    w = torch.from_numpy(golden["comp_w"])  # full coarse weights; the kernel uses [1:-1]
    z = torch.from_numpy(golden["comp_z"])
    u = None if det else torch.from_numpy(golden["pdf_u"])
    out = ops.sample_pdf(z.to(cuda), w.to(cuda), 128, det, u=None if det else u.to(cuda), debug=True)
    ref = O.sample_pdf(bins, w[..., 1:-1], 128, det, u)
    key = "pdf_det" if det else "pdf_u"
    np.testing.assert_array_equal(ref.samples.numpy(), golden[f"{key}_samples"])  # oracle pinned
    # CDF bit-exact: the normaliser is summed in torch CPU's order (common.h torch_row_sum), the
    # cumsum accumulated in fp64 like torch's
    np.testing.assert_array_equal(out["cdf"].cpu().numpy(), ref.cdf.numpy())
    # indices and samples bit-exact for identical CDF inputs: the oracle on the kernel's CDF
    s_ours, i_ours = O.samples_from_cdf(bins, out["cdf"].cpu(), ref.u)
    assert torch.equal(out["inds"].cpu().long(), i_ours)
    np.testing.assert_array_equal(out["samples"].cpu().numpy(), s_ours.numpy())
    zf_ref, _ = torch.sort(torch.cat([z, s_ours], -1), -1)
    np.testing.assert_array_equal(out["z_fine"].cpu().numpy(), zf_ref.numpy())
    # and so equal to the reference's own samples
    np.testing.assert_array_equal(out["samples"].cpu().numpy(), golden[f"{key}_samples"])


@pytest.mark.parametrize("Sc", [64, 41, 33, 10, 3])
def test_sample_pdf_cdf_bit_exact_random(cuda, ops, O, Sc):
    """The CDF -- and with it every importance sample -- bit for bit against torch CPU on
    weights of mixed magnitudes (a trained net's: a few near 1, most near 0), for every
    coarse-sample count the kernel supports down to 3: the normalising torch.sum's ATen order
    (8-lane vectors, ilp 4, scalar tail) covers full vectors, leftovers and tails."""
    g = torch.Generator().manual_seed(11 + Sc)
    R = 4096
    w = torch.rand(R, Sc, generator=g) ** 12 * torch.rand(R, 1, generator=g) * 4
    w[: R // 4] *= 1e-6  # near-empty rays: the 1e-5 floor dominates
    z = torch.sort(2 + 4 * torch.rand(R, Sc, generator=g), -1).values
    zmid = 0.5 * (z[..., 1:] + z[..., :-1])
    out = ops.sample_pdf(z.to(cuda), w.to(cuda), 128, True, debug=True)
    ref = O.sample_pdf(zmid, w[..., 1:-1], 128, True)
    np.testing.assert_array_equal(out["cdf"].cpu().numpy(), ref.cdf.numpy())
    np.testing.assert_array_equal(out["samples"].cpu().numpy(), ref.samples.numpy())
    assert torch.equal(out["inds"].cpu().long(), ref.inds)


# ---------------------------------------------------------------------------------- composite
def test_composite_forward(golden, cuda, ops):
    raw = torch.from_numpy(golden["comp_raw"]).to(cuda)
    z = torch.from_numpy(golden["comp_z"]).to(cuda)
    d = torch.from_numpy(golden["comp_d"]).to(cuda)
    rgb, depth, acc, w = ops.composite(raw, z, d, True)
    np.testing.assert_allclose(rgb.cpu().numpy(), golden["comp_rgb"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(depth.cpu().numpy(), golden["comp_depth"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(acc.cpu().numpy(), golden["comp_acc"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(w.cpu().numpy(), golden["comp_w"], rtol=0, atol=1e-6)


@pytest.mark.parametrize("S", [64, 192, 100])
def test_composite_backward(cuda, ops, O, S):
    g = torch.Generator().manual_seed(S)
    R = 96
    raw = (torch.randn(R, S, 4, generator=g) * 2).double().float()
    z = torch.sort(torch.rand(R, S, generator=g) * 4 + 2, -1).values
    d = torch.randn(R, 6, generator=g)
    gr = torch.randn(R, 3, generator=g)
    gd = torch.randn(R, generator=g)
    ga = torch.randn(R, generator=g)
    raw_c = raw.clone().requires_grad_(True)
    rgb, dep, acc, _ = O.composite(raw_c, z, d[:, 3:], True)
    (rgb * gr).sum().backward(retain_graph=True)
    ref1 = raw_c.grad.clone()
    raw_c.grad = None
    ((rgb * gr).sum() + (dep * gd).sum() + (acc * ga).sum()).backward()
    ref2 = raw_c.grad.clone()
    raw_g = raw.to(cuda).requires_grad_(True)
    rgb_g, dep_g, acc_g, _ = ops.composite(raw_g, z.to(cuda), d.to(cuda)[:, 3:], True)
    np.testing.assert_allclose(rgb_g.detach().cpu().numpy(), rgb.detach().numpy(), rtol=0, atol=1e-5)
    (rgb_g * gr.to(cuda)).sum().backward(retain_graph=True)
    np.testing.assert_allclose(raw_g.grad.cpu().numpy(), ref1.numpy(), rtol=1e-4, atol=1e-5)
    raw_g.grad = None
    ((rgb_g * gr.to(cuda)).sum() + (dep_g * gd.to(cuda)).sum() + (acc_g * ga.to(cuda)).sum()).backward()
    np.testing.assert_allclose(raw_g.grad.cpu().numpy(), ref2.numpy(), rtol=1e-4, atol=1e-4)


# ---------------------------------------------------------------------------------- MLP
@pytest.mark.parametrize("dtype,tol", [("fp32", 2e-5), ("bf16x3", 2e-5), ("bf16x6", 2e-5), ("bf16", 2e-2)])
def test_mlp_forward(golden, cuda, ops, packers, dtype, tol):
    pts = torch.from_numpy(golden["mlp_pts"]).to(cuda)
    vd = torch.from_numpy(golden["mlp_vd"]).to(cuda)
    for prefix, key in (("model", "mlp_raw_coarse"), ("model_fine", "mlp_raw_fine")):
        with torch.no_grad():
            raw = ops.mlp(packers[prefix], pts.reshape(-1, 3), vd, 8, dtype=dtype)
        np.testing.assert_allclose(raw.cpu().numpy().reshape(32, 8, 4), golden[key], rtol=0, atol=tol)


def test_mlp_bf16x6_is_fp32_class(cuda, ops, O):
    """The bf16x6 inference forward (x = hi + mid + lo, six bf16 products, fp32 accumulation; the coarse net
    of a bf16x3 / bf16x3f render) against an fp64 MLP on the trained net (golden trained_v2.npz), 20,000
    points inside the scene box: fp32-class (its largest error within 2x of the fp32 MFMA forward's; measured
    1.5e-4 vs 1.2e-4) and 6x closer than bf16x3 (9.3e-4).  bf16x6 refuses autograd and the density-only pass."""
    import os
    F = torch.nn.functional
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "trained_v2.npz"), allow_pickle=False)
    st = {k: torch.from_numpy(z[k]) for k in z.files}
    p = O.split_params(st, "model")
    g = torch.Generator().manual_seed(17)
    M, spd = 20000, 20
    pts = torch.rand(M, 3, generator=g) * 2.4 - 1.2
    vd = F.normalize(torch.randn(M // spd, 3, generator=g), dim=-1)
    pd = {k: (w.double(), b.double()) for k, (w, b) in p.items()}
    with torch.no_grad():
        d = vd.double()[torch.arange(M) // spd]
        ref = O.mlp(pd, O.positional_encoding(pts.double(), 10), O.positional_encoding(d, 4))
    params = [st[f"model.{n}"].to(cuda).contiguous() for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    err = {}
    for dt in ("fp32", "bf16x6", "bf16x3"):
        with torch.no_grad():
            raw = ops.mlp(packer, pts.to(cuda), vd.to(cuda), spd, dtype=dt)
        err[dt] = float((raw.double().cpu() - ref).abs().max())
    print(f"\nmax |raw - fp64 MLP|: {err}")
    assert err["bf16x6"] <= 2 * err["fp32"] + 1e-6, err
    assert err["bf16x6"] * 4 < err["bf16x3"], err
    with pytest.raises(RuntimeError, match="inference forward only"):
        ops.mlp(packer, pts[:64].to(cuda), vd[:4].to(cuda), 16, dtype="bf16x6", density_only=True)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16"])
def test_mlp_forward_large_and_density(cuda, ops, O, packers, seeded_state, dtype):
    g = torch.Generator().manual_seed(11)
    M = 5000  # not a multiple of the tile sizes
    pts = torch.rand(M, 3, generator=g) * 3 - 1.5
    vd = torch.nn.functional.normalize(torch.randn(M // 10, 3, generator=g), dim=-1)
    p = O.split_params(seeded_state, "model")
    with torch.no_grad():
        ref = O.network_forward(p, pts.reshape(M // 10, 10, 3), vd).reshape(M, 4)
        got = ops.mlp(packers["model"], pts.to(cuda), vd.to(cuda), 10, dtype=dtype).cpu()
        dens = ops.mlp(packers["model"], pts.to(cuda), None, 1, dtype=dtype, density_only=True).cpu()
    tol = 2e-2 if dtype == "bf16" else 2e-5
    np.testing.assert_allclose(got.numpy(), ref.numpy(), rtol=0, atol=tol)
    np.testing.assert_allclose(dens[:, 3].numpy(), ref[:, 3].numpy(), rtol=0, atol=tol)
    assert float(dens[:, :3].abs().max()) == 0.0


def _oracle_mlp_grads(O, seeded_state, pts, vd, gout, spd, dt):
    M = pts.shape[0]
    dirs = vd[:, None].expand(-1, spd, 3).reshape(M, 3)
    emb = torch.cat([O.positional_encoding(pts, 10), O.positional_encoding(dirs, 4)], -1).to(dt)
    prm = {k: v.to(dt).clone().requires_grad_(True) for k, v in seeded_state.items() if k.startswith("model.")}
    (O.mlp(O.split_params(prm, "model"), emb[:, :63], emb[:, 63:]) * gout.to(dt)).sum().backward()
    return {k[len("model."):]: v.grad.double() for k, v in prm.items()}


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3"])
def test_mlp_backward(cuda, ops, O, seeded_state, dtype):
    g = torch.Generator().manual_seed(12)
    M = 1000
    pts = torch.rand(M, 3, generator=g) * 3 - 1.5
    vd = torch.nn.functional.normalize(torch.randn(100, 3, generator=g), dim=-1)
    gout = torch.randn(M, 4, generator=g)
    ref = _oracle_mlp_grads(O, seeded_state, pts, vd, gout, 10, torch.float32)
    params = [seeded_state[f"model.{n}"].to(cuda).clone().requires_grad_(True) for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    raw = ops.mlp(packer, pts.to(cuda), vd.to(cuda), 10, dtype=dtype)
    (raw * gout.to(cuda)).sum().backward()
    for name, prm in zip(ops.NET_PARAM_NAMES, params):
        r = ref[name]
        gg = prm.grad.cpu().double()
        if dtype == "fp32":
            err = float((gg - r).abs().max()) / (float(r.abs().max()) + 1e-12)
            assert err < 1e-4, (name, err)
        else:
            # ~1e-5 relative pre-activations flip the ReLU masks of the few samples within that
            # of zero: each an O(1/M) change of single entries (up to 5e-3 of the largest one
            # measured); in norm the gradient holds to ~1e-3 (the masked test below pins the GEMMs;
            # bf16 is pinned there against its exact rounding model)
            rel = float((gg - r).norm() / (r.norm() + 1e-12))
            assert rel < 5e-3, (name, rel)


def _decode_masks(masks_u8, M):
    """ReLU masks [nblk, 9 groups, 64 lanes, 4 dwords] (group l < 8: layer l, group 8: the view
    layer; tile n in dword n >> 1, register rho at bit 8 (n & 1) + (rho >> 1) + 16 (rho & 1);
    lane l = sample 32 blk + (l & 31), register rho = feature acc_row(rho, l >> 5) of the tile)
    -> {tile: bool [M, 32]} with tile 8 l + n for the trunk and 64 + n for the view layer."""
    w = masks_u8.view(torch.int32).cpu().numpy().view(np.uint32).reshape(-1, 9, 64, 4)
    nblk = w.shape[0]
    out = np.zeros((nblk, 68, 32, 32), dtype=bool)  # [blk, tile, sample, feature]
    for t in range(68):
        grp, n = (t // 8, t % 8) if t < 64 else (8, t - 64)
        word = w[:, grp, :, n >> 1]  # [nblk, 64]
        for rho in range(16):
            bit = 8 * (n & 1) + (rho >> 1) + 16 * (rho & 1)
            b = ((word >> bit) & 1).astype(bool)
            for h in range(2):
                out[:, t, :, (rho & 3) + 8 * (rho >> 2) + 4 * h] = b[:, 32 * h:32 * h + 32]
    out = out.transpose(1, 0, 2, 3).reshape(68, -1, 32)[:, :M]
    return torch.from_numpy(out)


def _masked_mlp(p, x63, d27, mk):
    """oracle.mlp with each ReLU replaced by the kernel's own mask (identical branch choices)."""
    F = torch.nn.functional
    hmask = lambda tile0, n: torch.cat([mk[tile0 + j] for j in range(n)], 1).to(x63.dtype)  # noqa: E731
    h = x63
    for i in range(8):
        h = F.linear(h, *p[f"pts_linears.{i}"]) * hmask(8 * i, 8)
        if i == 4:
            h = torch.cat([x63, h], -1)
    alpha = F.linear(h, *p["alpha_linear"])
    feat = F.linear(h, *p["feature_linear"])
    hv = F.linear(torch.cat([feat, d27], -1), *p["views_linears.0"]) * hmask(64, 4)
    return torch.cat([F.linear(hv, *p["rgb_linear"]), alpha], -1)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_pe_fused_tiles(cuda, ops, O, seeded_state, dtype):
    """a4 directly: the positional encoding the fused forward generates (freq.py:7-32), read back
    from its training store -- tiles AT_X 0-1 (PE(xyz), 63 features + 1 zero) and AT_D 2 (PE(dir),
    27 + 5 zero) of each 32-sample block, block-major, chunk c of 64 lanes x 16 B holding
    registers 4c + e (fp32) / 8c + e (bf16; bf16x3: hi chunks, then lo), feature acc_row(rho,
    lane >> 5) of sample lane & 31 -- against the oracle's torch encoding of the same points.  fp32
    (libm sincosf of the exact x 2^k): within 2 ulp of 1.0 (2.4e-7), raw coordinates and padding
    exact; bf16 (v_sin_f32 after an f64 revolution reduction, then rounded to bf16): within bf16's
    relative half-ulp; bf16x3 (f64 revolution reduction + fp32 polynomial, split hi + lo): within
    2^-16 relative."""
    from nerf_amd._lib import lib, ptr, stream_of
    M, spd = 20010, 10
    g = torch.Generator().manual_seed(21)
    pts = torch.rand(M, 3, generator=g) * 8 - 4        # |x 2^9| up to 2048 rad
    vd = torch.nn.functional.normalize(torch.randn(-(-M // spd), 3, generator=g), dim=-1)
    params = [seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    code = ops.dtype_code(dtype)
    pc, vc = pts.to(cuda), vd.to(cuda)
    act = torch.zeros(lib().nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda)
    masks = torch.empty(lib().nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda)
    raw = torch.empty(M, 4, device=cuda)
    assert lib().nerf_mlp_fwd(ptr(packer.get(code, 0)), code, ptr(pc), ptr(vc), spd, None, M, 1, ptr(raw), ptr(act),
                              ptr(masks), stream_of(pc)) == 0
    torch.cuda.synchronize()
    dirs = vd[:, None].expand(-1, spd, 3).reshape(-1, 3)[:M]
    if dtype == "fp32":
        v = act.view(torch.float32).cpu()
        E, CH = 4, 4
    else:
        v = act.view(torch.bfloat16).float().cpu()
        E, CH = 8, (4 if dtype == "bf16x3" else 2)
    nblk = v.numel() // (79 * 32 * 32 * (2 if dtype == "bf16x3" else 1))
    v = v.reshape(nblk, 79, CH, 64, E)[:, :3]                      # [blk, tile, c, lane, e]
    if dtype == "bf16x3":                                           # hi (chunks 0, 1) + lo (2, 3)
        v = v[:, :, :2] + v[:, :, 2:]
        CH = 2
    dec = torch.zeros(nblk, 32, 96)                                 # [blk, sample, feature]
    for t in range(3):
        for c in range(CH):
            for e in range(E):
                rho = E * c + e
                for h in range(2):
                    f = 32 * t + (rho & 3) + 8 * (rho >> 2) + 4 * h
                    dec[:, :, f] = v[:, t, c, 32 * h:32 * h + 32, e]
    dec = dec.reshape(-1, 96)[:M]
    ref_x, ref_d = O.positional_encoding(pts, 10), O.positional_encoding(dirs, 4)
    got_x, got_d = dec[:, :63], dec[:, 64:91]
    assert float(dec[:, 63].abs().max()) == 0 and float(dec[:, 91:].abs().max()) == 0   # padding
    if dtype == "fp32":
        np.testing.assert_array_equal(got_x[:, :3].numpy(), ref_x[:, :3].numpy())
        np.testing.assert_array_equal(got_d[:, :3].numpy(), ref_d[:, :3].numpy())
        rtol, atol = 0.0, 2.4e-7
    elif dtype == "bf16":  # bf16's relative half-ulp (2^-9) of the rounded value, + v_sin_f32's ~1e-6
        rtol, atol = 2.0 ** -8, 2e-6
    else:  # hi + lo keeps 16 significant bits (2^-16 relative), + the polynomial's ~2 ulp
        rtol, atol = 2.0 ** -16, 1e-6
    np.testing.assert_allclose(got_x.numpy(), ref_x.numpy(), rtol=rtol, atol=atol)
    np.testing.assert_allclose(got_d.numpy(), ref_d.numpy(), rtol=rtol, atol=atol)


# measured max-entry errors against the rounding model: raw 1.2e-3 / 1.4e-3, gradients <= 5.9e-4
# (M = 20,010 / 131,101): fp32 accumulation order and operands within fp32 error of a bf16 tie
BF16_EMU_TOL = 3e-3


def _bf16_emulated_mlp(p, x63, d27, mk, gout, fwd_exact=False):
    """The bf16 kernels' arithmetic in fp64 (csrc/mlp.hip PBF16): every MFMA operand rounded to
    bf16 (RNE) where the kernel rounds it -- the PE tiles, the weights (fwd W, dX W^T), each
    layer's post-ReLU activation and the feature output, the output gradients d rgb / d alpha and
    each stage's masked pre-activation gradient dZ -- with the bias as the fp32 initial
    accumulator, the kernel's own ReLU masks ``mk`` and exact (fp64) accumulation.  Returns (raw,
    {param: grad}); dW = sum_m bf16(dZ) bf16(act), db = sum_m bf16(dZ).
    fwd_exact (bf16x3f): the forward is exact (fp64, fp32-class weights and activations, as the
    bf16x3 forward computes it) and only what it STORES for the backward is rounded to bf16 --
    the activations, the PE tiles -- while the backward is the bf16 one (bf16 W^T, bf16 dZ)."""
    bf = lambda t: t.to(torch.bfloat16).double()  # noqa: E731
    fr = (lambda t: t) if fwd_exact else bf  # rounding inside the forward  # noqa: E731
    hm = lambda tile0, n: torch.cat([mk[tile0 + j] for j in range(n)], 1).double()  # noqa: E731
    W = {k: bf(w.double()) for k, (w, b) in p.items()}
    Wf = {k: fr(w.double()) for k, (w, b) in p.items()}
    B = {k: b.double() for k, (w, b) in p.items()}
    xf, df_ = fr(x63.double()), fr(d27.double())
    ins, masks = [], []
    h = xf
    for i in range(8):
        n = f"pts_linears.{i}"
        ins.append(bf(h))
        m = hm(8 * i, 8)
        masks.append(m)
        h = fr((h @ Wf[n].t() + B[n]) * m)
        if i == 4:
            h = torch.cat([xf, h], -1)
    h7 = h
    alpha = h7 @ Wf["alpha_linear"].t() + B["alpha_linear"]
    feat = fr(h7 @ Wf["feature_linear"].t() + B["feature_linear"])
    vin_f = torch.cat([feat, df_], -1)
    mv = hm(64, 4)
    hv_f = fr((vin_f @ Wf["views_linears.0"].t() + B["views_linears.0"]) * mv)
    rgb = hv_f @ Wf["rgb_linear"].t() + B["rgb_linear"]
    raw = torch.cat([rgb, alpha], -1)
    h7, vin, hv = bf(h7), bf(vin_f), bf(hv_f)
    g = {}
    g_rgb, g_a = bf(gout[:, :3].double()), bf(gout[:, 3:].double())

    def put(name, dz, act):
        g[f"{name}.weight"] = dz.t() @ act
        g[f"{name}.bias"] = dz.sum(0)
    put("rgb_linear", g_rgb, hv)
    dzv = bf(g_rgb @ W["rgb_linear"]) * mv
    put("views_linears.0", dzv, vin)
    dfeat = bf(dzv @ W["views_linears.0"][:, :256])
    put("feature_linear", dfeat, h7)
    put("alpha_linear", g_a, h7)
    dz = bf(dfeat @ W["feature_linear"] + g_a @ W["alpha_linear"]) * masks[7]
    for i in range(7, -1, -1):
        n = f"pts_linears.{i}"
        put(n, dz, ins[i])
        if i == 0:
            break
        wt = W[n][:, 63:] if i == 5 else W[n]
        dz = bf(dz @ wt) * masks[i - 1]
    return raw, g


@pytest.mark.parametrize("dtype,M", [("fp32", 20010), ("bf16x3", 20010), ("bf16", 20010), ("bf16", 131101),
                                     ("bf16x3f", 20010)])
def test_mlp_backward_kernel_masks(cuda, ops, O, seeded_state, dtype, M):
    """Many dW sample chunks (the last partial) and a ragged final block, against an fp64
    oracle that takes the kernel's own ReLU masks: at these sizes a few pre-activations sit
    within fp32 rounding of 0, and any two fp32 evaluations (the oracle's own fp32 vs fp64
    included) pick different branches there -- forcing the branches isolates the GEMMs.
    fp32 and bf16x3 (16-bit split operands; measured <= 1.7e-5): 1e-4 of the largest entry.
    bf16: against the fp64 emulation of its own rounding (_bf16_emulated_mlp), raw and every
    gradient entry within BF16_EMU_TOL of the largest: what remains is fp32 accumulation order
    and the rare operand that sits within fp32 error of a bf16 rounding boundary.
    bf16x3f (bf16x3 forward, bf16 backward on the forward's bf16-rounded stores): raw within 1e-4
    of the exact forward, every gradient entry within BF16_EMU_TOL of its rounding model."""
    from nerf_amd._lib import lib, ptr, stream_of
    g = torch.Generator().manual_seed(12)
    spd = 10
    pts = torch.rand(M, 3, generator=g) * 3 - 1.5
    vd = torch.nn.functional.normalize(torch.randn(-(-M // spd), 3, generator=g), dim=-1)
    gout = torch.randn(M, 4, generator=g)
    params = [seeded_state[f"model.{n}"].to(cuda).clone().requires_grad_(True) for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    code = ops.dtype_code(dtype)
    # the kernel's masks: the same forward, with its training stores into our own buffers
    pc, vc = pts.to(cuda), vd.to(cuda)
    act = torch.empty(lib().nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda)
    masks = torch.empty(lib().nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda)
    raw0 = torch.empty(M, 4, device=cuda)
    assert lib().nerf_mlp_fwd(ptr(packer.get(code, 0)), code, ptr(pc), ptr(vc), spd, None, M, 1, ptr(raw0), ptr(act),
                              ptr(masks), stream_of(pc)) == 0
    raw = ops.mlp(packer, pc, vc, spd, dtype=dtype)
    (raw * gout.to(cuda)).sum().backward()
    torch.testing.assert_close(raw0, raw.detach(), rtol=0, atol=0)  # deterministic forward
    mk = _decode_masks(masks, M)

    dirs = vd[:, None].expand(-1, spd, 3).reshape(-1, 3)[:M]
    errs = {}
    if dtype in ("bf16", "bf16x3f"):
        emb = torch.cat([O.positional_encoding(pts, 10), O.positional_encoding(dirs, 4)], -1)
        sp = O.split_params({k: v for k, v in seeded_state.items() if k.startswith("model.")}, "model")
        ref_raw, ref_g = _bf16_emulated_mlp(sp, emb[:, :63], emb[:, 63:], mk, gout, fwd_exact=dtype == "bf16x3f")
        got = raw.detach().cpu().double()
        if dtype == "bf16x3f":
            np.testing.assert_allclose(got.numpy(), ref_raw.numpy(), rtol=0, atol=1e-4)
        errs["raw"] = float((got - ref_raw).abs().max()) / float(ref_raw.abs().max())
        for name, prm_g in zip(ops.NET_PARAM_NAMES, params):
            r = ref_g[name].reshape(prm_g.shape)
            errs[name] = float((prm_g.grad.cpu().double() - r).abs().max()) / (float(r.abs().max()) + 1e-30)
        print(f"\n{dtype} M={M} max-entry errors vs the bf16 rounding model:", {k: f"{v:.2e}" for k, v in errs.items()})
        assert max(errs.values()) < BF16_EMU_TOL, errs
        return
    emb = torch.cat([O.positional_encoding(pts, 10), O.positional_encoding(dirs, 4)], -1).double()
    prm = {k: v.double().clone().requires_grad_(True) for k, v in seeded_state.items() if k.startswith("model.")}
    ref = _masked_mlp(O.split_params(prm, "model"), emb[:, :63], emb[:, 63:], mk)
    (ref * gout.double()).sum().backward()
    np.testing.assert_allclose(raw.detach().cpu().double().numpy(), ref.detach().numpy(), rtol=0, atol=1e-4)
    for name, prm_g in zip(ops.NET_PARAM_NAMES, params):
        r = prm[f"model.{name}"].grad
        gg = prm_g.grad.cpu().double()
        err = errs[name] = float((gg - r).abs().max()) / (float(r.abs().max()) + 1e-30)
        assert err < 1e-4, (name, err)
    print(f"\n{dtype} M={M} max-entry errors:", {k: f"{v:.2e}" for k, v in errs.items()})


# ---------------------------------------------------------------------------------- grid
def test_bf16x3f_stores_are_the_bf16x3_hi_halves(cuda, ops, seeded_state):
    """bf16x3f's training forward (csrc/mlp.hip FwdWave HALF) is the bf16x3 forward with bf16
    stores: raw and the ReLU masks bit-identical to bf16x3's, and every stored tile-block equal to
    the hi half (the first two 1 KiB chunks) of bf16x3's 4 KiB tile-block, in the bf16 layout the
    bf16 dX / dW kernels read."""
    from nerf_amd._lib import lib, ptr, stream_of
    g = torch.Generator().manual_seed(21)
    M, spd = 20010, 10
    pts = (torch.rand(M, 3, generator=g) * 3 - 1.5).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(-(-M // spd), 3, generator=g), dim=-1).to(cuda)
    params = [seeded_state[f"model.{n}"].to(cuda).clone() for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    out = {}
    for code in (ops.BF16X3, ops.BF16X3F):
        act = torch.zeros(lib().nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda)
        masks = torch.zeros(lib().nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda)
        raw = torch.empty(M, 4, device=cuda)
        assert lib().nerf_mlp_fwd(ptr(packer.get(code, 0)), code, ptr(pts), ptr(vd), spd, None, M, 1, ptr(raw), ptr(act),
                                  ptr(masks), stream_of(pts)) == 0
        out[code] = (raw, act, masks)
    torch.cuda.synchronize()
    (r3, a3, m3), (rf, af, mf) = out[ops.BF16X3], out[ops.BF16X3F]
    assert torch.equal(r3, rf) and torch.equal(m3, mf)
    nblk = lib().nerf_mlp_padded_samples(M) // 32
    assert af.numel() * 2 == a3.numel() == nblk * 79 * 4096
    hi = a3.view(nblk, 79, 4, 1024)[:, :, :2]
    assert torch.equal(hi.reshape(-1), af)
    # and the bf16x3f packs are the bf16x3 forward pack and the bf16 backward pack
    assert torch.equal(packer.get(ops.BF16X3F, 0), packer.get(ops.BF16X3, 0))
    assert torch.equal(packer.get(ops.BF16X3F, 1), packer.get(ops.BF16, 1))


def test_grid_index_bit_exact(golden, cuda, ops):
    pts = torch.from_numpy(golden["grid_pts"]).to(cuda)
    idx, _ = ops.grid_index(pts, None, 128)
    np.testing.assert_array_equal(idx.cpu().numpy(), golden["grid_idx"])


MARCH_CASES = [(d, r, m, True, False, 6.0) for d in (0.02, 0.3, "blob") for r in (128, 512, 1024) for m in (True, False)]
MARCH_CASES += [(d, 128, True, False, False, 6.0) for d in (0.02, 0.3, "blob")]   # the two-pass form
MARCH_CASES += [(d, 128, True, p, True, 6.0) for d in (0.3, "blob") for p in (True, False)]  # buffer overflow
MARCH_CASES += [(d, r, True, True, False, 24.0) for d in (0.3, "blob") for r in (128, 1024)]  # far bound > 8


@pytest.mark.parametrize("density,res,macro,one_pass,tight,far", MARCH_CASES)
def test_march_gather_empty_cell_skip_exact(cuda, ops, density, res, macro, one_pass, tight, far):
    """The march gather skips the steps that provably stay in an empty cell (march.hip,
    march_skip_empty).  Against brute force -- the occupancy of EVERY step's point o + t d
    (volume_renderer.py:298-309: clamp, normalise, x127, truncate) -- the one-round gather with
    K = all steps emits exactly the occupied (ray, step) pairs, in step order: rays from outside
    the box and from inside, axis-aligned direction components (d = 0), sparse and dense grids,
    at the config's res 128 and at 512 / 1024 (where 1e-3 of a cell alone would approach the fp32
    error of the points; march.hip's margin has an absolute floor), with and without the macro
    grid (whole empty 8^3 blocks crossed in one skip; 'blob' = an object in empty space).  The
    one-pass form writes the points from the runs its counting walk recorded (16 per lane, then
    the walk again: the dense grids' rays have far more runs) and must equal the two-pass form;
    'tight' gives the round half the room it needs: every reserved position below cap holds its
    ray's next occupied step, the overflowing rays keep their start step and gather again.
    far = 24: a t table past 8, origins ~12 out and |d| = 0.5, so |t d| ~ 12 at the
    box: the skip margin's absolute floor must grow with the table's largest t."""
    from nerf_amd._lib import lib, ptr, stream_of
    g = torch.Generator().manual_seed(31)
    N = 3000
    dens = 0.3 if density == "blob" else density
    if res == 128:
        grid = (torch.rand(res, res, res, generator=g) < dens)
    else:  # (finer grids drawn on the device: a 1024^3 host draw is slow)
        gd_ = torch.Generator(device=cuda).manual_seed(31 + res)
        grid = torch.rand(res, res, res, generator=gd_, device=cuda) < dens
    grid[:, :, :40 * res // 128] = False              # long empty runs
    if density == "blob":  # an object in empty space: whole empty 8^3 blocks around it (macro skip)
        c = torch.arange(res, device=grid.device, dtype=torch.float32) - res / 2
        r2 = c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2
        grid &= r2 < (0.3 * res) ** 2
    o = torch.cat([torch.randn(N // 2, 3, generator=g) * 0.3 + torch.tensor([0.0, 0.0, 4.0]),
                   torch.rand(N - N // 2, 3, generator=g) * 2 - 1])
    tgt = torch.rand(N, 3, generator=g) * 2.4 - 1.2
    d = tgt - o
    if far > 8.0:
        o[: N // 2] += torch.tensor([0.0, 0.0, 8.0])
        d = tgt - o
        d = d / d.norm(dim=1, keepdim=True) * 0.5
    d[::7, 0] = 0.0                                   # axis-aligned components
    d[::11, 1] = 0.0
    rays = torch.cat([o, d], 1).float().to(cuda).contiguous()
    t_table = ops.device_table("arange", 2.0, far, 0.005, cuda)
    S = t_table.numel()
    # brute force: every step's point, the lookup of grid_index
    pts = rays[:, None, :3] + t_table[None, :, None] * rays[:, None, 3:]
    _, occ = ops.grid_index(pts.reshape(-1, 3), grid.to(cuda), res, want_idx=False)
    occ = occ.reshape(N, S).bool().cpu()
    # one gather round, K = S
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=cuda)  # noqa: E731
    T, rgb, dep, acc = f(N), f(N, 3), f(N), f(N)
    nxt, start, off, cnt = (f(N, dt=torch.int32) for _ in range(4))
    if one_pass:
        start = None
    alive, exh = f(N, dt=torch.uint8), f(N, dt=torch.uint8)
    counters = torch.zeros(2, dtype=torch.int32, device=cuda)
    evaluated = torch.zeros(1, dtype=torch.int64, device=cuda)
    cap = int(occ.sum()) // 2 if tight else int(occ.sum()) + 16
    out_ray, out_step, out_pts = f(cap, dt=torch.int32), f(cap, dt=torch.int32), f(cap, 3)
    s = stream_of(rays)
    L = lib()
    assert L.nerf_march_init(ptr(T), ptr(rgb), ptr(dep), ptr(acc), ptr(nxt), ptr(alive), ptr(exh), N, s) == 0
    bb = ops._bbox_arr(ops.SCENE_BBOX)
    gd = grid.to(device=cuda, dtype=torch.uint8).contiguous()
    mg = None
    if macro:
        mg = torch.empty(L.nerf_march_macro_bytes(res), dtype=torch.uint8, device=cuda)
        assert L.nerf_march_macro(ptr(gd), res, ptr(mg), s) == 0
        m = res // 8
        ref_macro = gd.reshape(m, 8, m, 8, m, 8).amax(dim=(1, 3, 5)).reshape(-1)
        assert torch.equal(mg, (ref_macro > 0).to(torch.uint8))
    assert L.nerf_march_gather(ptr(rays), N, ptr(t_table), S, ptr(gd), res, ptr(mg), bb, S, S, 0.0, ptr(T), ptr(rgb), ptr(dep),
                               ptr(acc), ptr(nxt), ptr(alive), ptr(exh), ptr(counters), ptr(evaluated), ptr(start),
                               ptr(out_ray), ptr(out_step), ptr(out_pts), ptr(off), ptr(cnt), cap, s) == 0
    n_pts = int(counters[0])
    assert n_pts == int(occ.sum())
    n_written = min(n_pts, cap)
    assert int(evaluated[0]) == n_written
    c, o_, nx = cnt.cpu(), off.cpu(), nxt.cpu()
    steps, ray_ids = out_step[:n_written].cpu(), out_ray[:n_written].cpu()
    written = 0
    for r in range(N):
        want = torch.nonzero(occ[r]).flatten().int()
        k = int(c[r])
        if k < 0 or (tight and k == 0 and want.numel() > 0):  # overflowed: the part below cap, not composited
            assert int(o_[r]) + want.numel() > cap and int(nx[r]) == 0, r
            k = -k
            want = want[:k]
        else:
            assert k == want.numel(), r
        got = steps[int(o_[r]):int(o_[r]) + k]
        assert torch.equal(got, want), r
        assert bool((ray_ids[int(o_[r]):int(o_[r]) + k] == r).all())
        written += k
    assert written == n_written
    np.testing.assert_array_equal(out_pts[:n_written].cpu().numpy(),
                                  pts.cpu()[ray_ids.long(), steps.long()].numpy())


def test_adam_matches_torch(cuda, ops):
    g = torch.Generator().manual_seed(3)
    n = 10007
    p0 = torch.randn(n, generator=g)
    p_ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([p_ref], lr=5e-4, eps=1e-8)
    p = p0.clone().to(cuda)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for step in range(1, 6):
        gr = torch.randn(n, generator=g) * 60
        p_ref.grad = gr.clone()
        torch.nn.utils.clip_grad_value_([p_ref], 40)
        opt.step()
        gg = gr.to(cuda)
        ops.adam_step(p, gg, m, v, 5e-4, step, clip_value=40.0)
    np.testing.assert_allclose(p.cpu().numpy(), p_ref.detach().numpy(), rtol=0, atol=1e-6)


# ---------------------------------------------------------------------------------- evaluator
@pytest.mark.parametrize("H,W,noise", [(800, 800, 0.05), (37, 53, 0.3), (64, 64, 0.0)])
def test_image_metrics_match_host_evaluator(cuda, ops, H, W, noise):
    """GPU PSNR/SSIM (csrc/metrics.hip) against the evaluator's numpy definitions
    (src/evaluators/nerf.py, the reference's nerf.py:23-45 restated): SSIM to 1e-9, PSNR to
    1e-4 dB (float32 vs float64 mean of the squared errors)."""
    from src.evaluators.nerf import psnr_metric, ssim_metric_uint8
    g = torch.Generator().manual_seed(H * W)
    gt = torch.rand(H, W, 3, generator=g)
    pred = (gt + noise * torch.randn(H, W, 3, generator=g)).clamp(0.0, 1.0)
    if noise == 0.0:
        pred[5:9, 7:11] = 0.5  # not identical: finite PSNR
    psnr, ssim = ops.image_metrics(pred.to(cuda), gt.to(cuda))
    p_np, g_np = pred.numpy(), gt.numpy()
    ref_psnr = psnr_metric(p_np, g_np)
    ref_ssim = ssim_metric_uint8((p_np * 255).astype(np.uint8), (g_np * 255).astype(np.uint8))
    assert abs(psnr - ref_psnr) < 1e-4, (psnr, ref_psnr)
    assert abs(ssim - ref_ssim) < 1e-9, (ssim, ref_ssim)


@pytest.mark.parametrize("M", [131101, 786432])
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3", "bf16x3f"])
def test_training_kernels_bitwise_deterministic(cuda, ops, seeded_state, dtype, M):
    """The training forward, dX and deterministic dW run twice on the same inputs write the same bytes: raw,
    activation / mask / dz stores and the gradient, at a ragged size and at the fine net's config-3 launch.
    The weight ring's hand-offs are counted waits and barriers the compiler cannot see (csrc/mlp.hip); a late
    LDS read or an early DMA would show here as run-to-run differences.  (Round 5's finish-part sweep did see
    them -- NERF_FINISH_PARTS_BF16 = 2 / 8 -- from an inline-asm VGPR write racing an MFMA's write-back and a
    clamped finish part landing after the MFMA that reads its pair; both are now refused at build time:
    tools/asm_check.py, FinishSchedule, tests/test_finish_schedule.py.)"""
    from nerf_amd._lib import check, lib, ptr, stream_of
    L = lib()
    g = torch.Generator().manual_seed(31)
    code = ops.dtype_code(dtype)
    packer = ops.PackedMLP([seeded_state[f"model.{n}"].to(cuda).contiguous() for n in ops.NET_PARAM_NAMES])
    pts = (torch.rand(M, 3, generator=g) * 3 - 1.5).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(M // 9 + 1, 3, generator=g), dim=-1).to(cuda)
    d_raw = (torch.randn(M, 4, generator=g) * 1e-2).to(cuda)
    s = stream_of(pts)
    outs = []
    for _ in range(2):
        b = dict(raw=torch.zeros(M, 4, device=cuda),
                 act=torch.zeros(L.nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda),
                 masks=torch.zeros(L.nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda),
                 dz=torch.zeros(L.nerf_mlp_dz_bytes(code, M), dtype=torch.uint8, device=cuda),
                 grad=torch.zeros(L.nerf_mlp_net_params(), device=cuda))
        ws = torch.empty(L.nerf_mlp_dw_workspace_bytes(code, M), dtype=torch.uint8, device=cuda)
        check(L.nerf_mlp_fwd(ptr(packer.get(code, 0)), code, ptr(pts), ptr(vd), 9, None, M, 1, ptr(b["raw"]),
                             ptr(b["act"]), ptr(b["masks"]), s), "fwd")
        check(L.nerf_mlp_bwd_dx(ptr(packer.get(code, 1)), code, ptr(d_raw), M, ptr(b["masks"]), ptr(b["dz"]), s), "dx")
        check(L.nerf_mlp_bwd_dw_ws(code, M, ptr(b["act"]), ptr(b["dz"]), ptr(b["grad"]), ptr(ws), s), "dw")
        outs.append(b)
    torch.cuda.synchronize()
    for k in ("raw", "act", "masks", "dz", "grad"):
        assert torch.equal(outs[0][k], outs[1][k]), (dtype, k)
    if dtype != "fp32":  # (fp32 stores fp32 tiles: the bf16-pair check below does not apply)
        _assert_masks_implied_by_act(outs[0]["act"], outs[0]["masks"], M)


def _assert_masks_implied_by_act(act, masks, M):
    """Every stored ReLU mask bit equals "the stored post-ReLU activation (its bf16 hi half) is non-zero":
    mask dword n >> 1 of layer group l, bit 8 (n & 1) + (rho >> 1) + 16 (rho & 1) for register rho of tile n
    (csrc/mlp.hip mask_bit, mlp_tables.h ActTile).  The round-5 mask race broke exactly this relation."""
    nblk = (M + 255) // 256 * 8
    nch = act.numel() // (nblk * 79 * 1024)  # chunks per stored tile-block: 2 (bf16 / bf16 halves) or 4 (hi, lo)
    a = act.view(torch.int16).view(nblk, 79, nch, 64, 8)[:, :, :2]  # the bf16 (hi) chunks
    got = masks.view(torch.int32).view(nblk, 9, 64, 4).to(torch.int64) & 0xFFFFFFFF
    exp = torch.zeros_like(got)
    rho = torch.arange(16, device=act.device)
    bitpos = (rho >> 1) + 16 * (rho & 1)
    for grp in range(9):
        for n in range(8 if grp < 8 else 4):
            tau = 3 + 8 * grp + n if grp < 8 else 75 + n
            nz = (a[:, tau] != 0).permute(0, 2, 1, 3).reshape(nblk, 64, 16).to(torch.int64)
            exp[:, grp, :, n >> 1] |= (nz << (bitpos + 8 * (n & 1))).sum(-1)
    bad = (exp != got).sum(dim=(0, 2, 3))
    assert int(bad.sum()) == 0, f"mask dwords not implied by the stored activations, per layer group: {bad.tolist()}"


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3", "bf16x3f", "bf16x6"])
def test_mlp_ragged_sizes_row_independent(cuda, ops, seeded_state, dtype):
    """Ragged launch sizes (1, 31, 32, 33, 255, 257, 4133 samples: partial 32-sample wave blocks and
    256-sample workgroups): every sample's raw output is its row of the 4,133-sample launch, bit for bit
    (the MLP is row-independent; padding rows never leak into real ones)."""
    g = torch.Generator().manual_seed(29)
    big = 4133
    pts = (torch.rand(big, 3, generator=g) * 3 - 1.5).to(cuda)
    ndir = 97
    vd = torch.nn.functional.normalize(torch.randn(ndir, 3, generator=g), dim=-1).to(cuda)
    di = torch.randint(0, ndir, (big,), generator=g, dtype=torch.int32).to(cuda)
    packer = ops.PackedMLP([seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES])
    with torch.no_grad():
        ref = ops.mlp(packer, pts, vd, 1, di, dtype)
        for m in (1, 31, 32, 33, 255, 257):
            got = ops.mlp(packer, pts[:m].contiguous(), vd, 1, di[:m].contiguous(), dtype)
            assert torch.equal(got, ref[:m]), (dtype, m)


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_mlp_rows_independent_of_position(cuda, ops, seeded_state, dtype):
    """A sample's raw output does not depend on its position in the launch: 4,133 points evaluated as they are
    and through a random permutation of the rows (dir_index permuted along) give the same bits after
    un-permuting, through ops.mlp and through ops.mlp_count (the count read on the device).  The round march
    relies on it: a round's buffer holds a ray's points wherever the reservation put them
    (test_gpu_march_rounds.py::test_ops_march_round_options_change_no_bit)."""
    g = torch.Generator().manual_seed(41)
    M, ndir = 4133, 97
    pts = (torch.rand(M, 3, generator=g) * 3 - 1.5).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(ndir, 3, generator=g), dim=-1).to(cuda)
    di = torch.randint(0, ndir, (M,), generator=g, dtype=torch.int32).to(cuda)
    perm = torch.randperm(M, generator=g).to(cuda)
    assert not torch.equal(perm, torch.arange(M, device=cuda))
    p_pts, p_di = pts[perm].contiguous(), di[perm].contiguous()
    packer = ops.PackedMLP([seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES])
    count = torch.tensor([M, 0], dtype=torch.int32, device=cuda)

    def unpermute(raw):
        out = torch.empty_like(raw)
        out[perm] = raw
        return out

    with torch.no_grad():
        ref = ops.mlp(packer, pts, vd, 1, di, dtype)
        assert torch.equal(unpermute(ops.mlp(packer, p_pts, vd, 1, p_di, dtype)), ref), dtype
        ref = ops.mlp_count(packer, pts, vd, di, count, torch.full((M, 4), float("nan"), device=cuda), dtype)
        assert not bool(torch.isnan(ref).any())
        raw = ops.mlp_count(packer, p_pts, vd, p_di, count, torch.full((M, 4), float("nan"), device=cuda), dtype)
        assert torch.equal(unpermute(raw), ref), dtype


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3", "bf16x3f", "bf16x6"])
def test_pack_plan_gather_matches_direct_pack(cuda, ops, seeded_state, dtype):
    """nerf_mlp_pack gathers through its cached pack plan when the 24 parameters lie back to back
    (FusedAdam's flat buffer) and walks the units directly otherwise: byte-identical packs, both
    directions (csrc/mlp.hip pack_plan_kernel / pack_gather_kernel / pack_kernel)."""
    import ctypes
    from nerf_amd._lib import check, lib, ptr, stream_of
    L = lib()
    params = [seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES]
    offs = [L.nerf_mlp_param_offset(i) for i in range(24)]
    flat = torch.cat([p.reshape(-1) for p in params])
    assert offs == [sum(p.numel() for p in params[:i]) for i in range(24)]
    views = [flat[o:o + p.numel()] for o, p in zip(offs, params)]
    gapped = torch.zeros(flat.numel() + 16 * 24, device=cuda)   # the same values, 16 floats apart
    sep = []
    for i, p in enumerate(params):
        v = gapped[offs[i] + 16 * i:offs[i] + 16 * i + p.numel()]
        v.copy_(p.reshape(-1))
        sep.append(v)
    code = ops.dtype_code(dtype)
    for d in ((0,) if dtype == "bf16x6" else (0, 1)):
        outs = []
        for ps in (views, sep):
            arr = ctypes.cast((ctypes.c_void_p * 24)(*[p.data_ptr() for p in ps]), ctypes.c_void_p)
            buf = torch.full((L.nerf_mlp_packed_bytes(code, d),), 0xAB, dtype=torch.uint8, device=cuda)
            check(L.nerf_mlp_pack(arr, code, ptr(buf if d == 0 else None), ptr(buf if d == 1 else None),
                                  stream_of(flat)), "pack")
            outs.append(buf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]), (dtype, d)


@pytest.mark.parametrize("dtype", ["fp32", "bf16x3", "bf16", "bf16x3f"])
def test_mlp_dw_deterministic(cuda, ops, seeded_state, dtype):
    """dW with the workspace (per-item partials, fixed-order reduce) is bit-identical run to
    run and equal, to fp32 summation-order rounding, to the atomic accumulation."""
    from nerf_amd._lib import check, lib, ptr, stream_of
    g = torch.Generator().manual_seed(21)
    M = 70001
    code = ops.dtype_code(dtype)
    params = [seeded_state[f"model.{n}"].to(cuda).contiguous() for n in ops.NET_PARAM_NAMES]
    packer = ops.PackedMLP(params)
    pts = (torch.rand(M, 3, generator=g) * 3 - 1.5).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(M // 7 + 1, 3, generator=g), dim=-1).to(cuda)
    L = lib()
    act = torch.empty(L.nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda)
    masks = torch.empty(L.nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda)
    dz = torch.empty(L.nerf_mlp_dz_bytes(code, M), dtype=torch.uint8, device=cuda)
    raw = torch.empty(M, 4, device=cuda)
    s = stream_of(pts)
    check(L.nerf_mlp_fwd(ptr(packer.get(code, 0)), code, ptr(pts), ptr(vd), 7, None, M, 1, ptr(raw), ptr(act),
                         ptr(masks), s), "fwd")
    d_raw = torch.randn(M, 4, generator=g).to(cuda)
    check(L.nerf_mlp_bwd_dx(ptr(packer.get(code, 1)), code, ptr(d_raw), M, ptr(masks), ptr(dz), s), "dx")
    ws = torch.empty(L.nerf_mlp_dw_workspace_bytes(code, M), dtype=torch.uint8, device=cuda)
    outs = []
    for use_ws in (True, True, False):
        grad = torch.zeros(L.nerf_mlp_net_params(), device=cuda)
        check(L.nerf_mlp_bwd_dw_ws(code, M, ptr(act), ptr(dz), ptr(grad), ptr(ws) if use_ws else None, s), "dw")
        outs.append(grad.cpu())
    assert torch.equal(outs[0], outs[1])
    scale = float(outs[2].abs().max())
    assert float((outs[0] - outs[2]).abs().max()) <= 1e-5 * scale


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "bf16x3"])
def test_mlp_fwd_count_matches_fwd(cuda, ops, seeded_state, dtype):
    """nerf_mlp_fwd_count (the grid march's launch: sample count read on the device, a persistent
    grid looping over the sample blocks) is bit-identical to nerf_mlp_fwd on the first
    min(*M_dev, cap) points, for a count below the cap, above it, and zero (no point written)."""
    g = torch.Generator().manual_seed(41)
    cap = 50000
    pts = (torch.rand(cap, 3, generator=g) * 3 - 1.5).to(cuda)
    ndir = 777
    vd = torch.nn.functional.normalize(torch.randn(ndir, 3, generator=g), dim=-1).to(cuda)
    di = torch.randint(0, ndir, (cap,), generator=g, dtype=torch.int32).to(cuda)
    packer = ops.PackedMLP([seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES])
    for m in (12345, cap + 999, 0):
        M_dev = torch.tensor([m], dtype=torch.int32, device=cuda)
        raw = torch.full((cap, 4), float("nan"), device=cuda)
        ops.mlp_count(packer, pts, vd, di, M_dev, raw, dtype)
        n = min(m, cap)
        with torch.no_grad():
            ref = ops.mlp(packer, pts[:n], vd, 1, di[:n], dtype) if n else torch.empty(0, 4, device=cuda)
        torch.testing.assert_close(raw[:n], ref, rtol=0, atol=0)
        assert bool(torch.isnan(raw[n:]).all())  # nothing past the device count is written


@pytest.mark.parametrize("Sc,Ni", [(64, 128), (63, 128), (33, 64), (3, 7), (17, 1)])
@pytest.mark.parametrize("det", [True, False])
def test_composite_pdf_fused_equals_separate(cuda, ops, det, Sc, Ni):
    """ops.composite_sample_pdf (one launch: coarse compositing + importance sampling + merge,
    the weights handed over in registers) is bit-identical to composite() then sample_pdf(),
    forward and backward (volume_renderer.py:197-221).  Every coarse-sample count the renderer
    sends to the fused kernel (3 <= Sc <= 64): Sc < 64 leaves lanes Sc..63 without a sample (the
    l < Sc guard; the weight shuffled from lane l + 1 is used only for l < Sc - 2), and Ni down
    to one importance sample."""
    g = torch.Generator().manual_seed(41 + Sc + Ni)
    R = 1000
    o = torch.randn(R, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 4.0])
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 1.3
    rays = torch.cat([o, d], 1).to(cuda)
    z, _, _ = ops.sample_stratified(rays, 2.0, 6.0, Sc, not det, seed=5, offset=8)
    raw = (torch.randn(R, Sc, 4, generator=g) * 2).to(cuda).requires_grad_(True)
    raw2 = raw.detach().clone().requires_grad_(True)
    rgb, dep, acc, w = ops.composite(raw, z, rays[:, 3:6], True)
    pdf = ops.sample_pdf(z, w, Ni, det=det, seed=5, offset=9, rays=rays)
    rgb2, dep2, acc2, pdf2 = ops.composite_sample_pdf(raw2, z, rays, True, Ni, det=det, seed=5, offset=9)
    for a, b in ((rgb, rgb2), (dep, dep2), (acc, acc2), (pdf["z_fine"], pdf2["z_fine"]),
                 (pdf["pts_fine"], pdf2["pts_fine"])):
        assert torch.equal(a, b)
    gr = torch.randn(R, 3, generator=g).to(cuda)
    ((rgb * gr).sum() + dep.sum() + 0.5 * acc.sum()).backward()
    ((rgb2 * gr).sum() + dep2.sum() + 0.5 * acc2.sum()).backward()
    assert torch.equal(raw.grad, raw2.grad)


def test_composite_pdf_fragile_flag(cuda, ops):
    """nerf_composite_pdf_fragile (round 6): its rgb / depth / acc / z_fine / pts_fine are composite_sample_pdf's
    at det bit for bit, and its flag is exactly the documented rule, recomputed here from the CDF and the bins
    (ops.sample_pdf debug outputs): some u = linspace(0, 1, Ni) within rel_tol * min(c, 1 - c) + abs_tol of a
    bracketing entry c = cdf[k], k >= 1 (not the last entry against u = 1), or a den (cdf[above] - cdf[below],
    below != above) within den_tol of the 1e-5 switch (volume_renderer.py:115-126), or u = 1 with the last entry
    within abs_tol of 1 and the last interval below 1e-5 + den_tol."""
    g = torch.Generator().manual_seed(77)
    R, Sc, Ni = 2000, 64, 128
    o = torch.randn(R, 3, generator=g) * 0.2 + torch.tensor([0.0, 0.0, 4.0])
    d = torch.nn.functional.normalize(torch.randn(R, 3, generator=g), dim=-1) * 1.3
    rays = torch.cat([o, d], 1).to(cuda)
    z, _, _ = ops.sample_stratified(rays, 2.0, 6.0, Sc, False)
    raw = (torch.randn(R, Sc, 4, generator=g) * 2).to(cuda)
    raw[: R // 2, :, 3] -= 6.0  # (half the rays nearly empty: CDF entries crowd near 0 / the 1e-5 switch)
    rel, ab, dt = 1e-3, 1.2e-7, 2e-8
    with torch.no_grad():
        rgb, dep, acc, pdf = ops.composite_sample_pdf(raw, z, rays, True, Ni, det=True)
        rgb2, dep2, acc2, pdf2, frag = ops.composite_sample_pdf_fragile(raw, z, rays, True, Ni, rel, ab, dt)
        _, _, _, w = ops.composite(raw, z, rays[:, 3:6], True)
        dbg = ops.sample_pdf(z, w, Ni, det=True, debug=True)
    for a, b in ((rgb, rgb2), (dep, dep2), (acc, acc2), (pdf["z_fine"], pdf2["z_fine"]),
                 (pdf["pts_fine"], pdf2["pts_fine"])):
        assert torch.equal(a, b)
    cdf, ind = dbg["cdf"].double().cpu(), dbg["inds"].long().cpu()
    nb = Sc - 1
    u = torch.linspace(0, 1, Ni, dtype=torch.float32).double()
    tau = (rel * torch.minimum(cdf, 1 - cdf) + ab).float().double()
    exp = torch.zeros(R, dtype=torch.bool)
    for r in range(R):
        for i in range(Ni):
            k = int(ind[r, i])
            end = u[i] >= 1.0
            lo, hi = max(k - 1, 0), min(k, nb - 1)
            if k - 1 >= 1 and not (end and k - 1 == nb - 1) and u[i] - cdf[r, k - 1] < tau[r, k - 1]:
                exp[r] = True
            if k <= nb - 1 and not (end and k == nb - 1) and cdf[r, k] - u[i] <= tau[r, k]:
                exp[r] = True
            if lo != hi and abs(float(torch.tensor(cdf[r, hi] - cdf[r, lo], dtype=torch.float32)) - 1e-5) <= dt:
                exp[r] = True
            if end and abs(float(cdf[r, nb - 1]) - 1.0) <= ab and \
                    float(torch.tensor(cdf[r, nb - 1] - cdf[r, nb - 2], dtype=torch.float32)) < 1e-5 + dt:
                exp[r] = True
    got = frag.bool().cpu()
    # (the kernel compares in fp32, this in fp64: allow the few rays whose margin equals the tolerance to the ulp)
    assert int((got != exp).sum()) <= 2, (int(got.sum()), int(exp.sum()))
    assert 0 < int(got.sum()) < R


def test_mse_pair_matches_torch(cuda, ops):
    """ops.mse_pair = nn.MSELoss()(c, gt) + nn.MSELoss()(f, gt) (src/train/trainers/nerf.py:21-29):
    the losses within fp32 rounding of torch's (fp64 sums here), the gradients of the total (and of
    each loss) equal to torch's autograd."""
    g = torch.Generator().manual_seed(42)
    n = 4096
    c0, f0, gt = (torch.rand(n, 3, generator=g).to(cuda) for _ in range(3))
    c, f = c0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    lc, lf, tot = ops.mse_pair(c, f, gt)
    (tot + 0.25 * lc).backward()
    c1, f1 = c0.clone().requires_grad_(True), f0.clone().requires_grad_(True)
    rc, rf = torch.nn.functional.mse_loss(c1, gt), torch.nn.functional.mse_loss(f1, gt)
    ((rc + rf) + 0.25 * rc).backward()
    np.testing.assert_allclose([float(lc), float(lf), float(tot)], [float(rc), float(rf), float(rc + rf)], rtol=1e-6)
    torch.testing.assert_close(c.grad, c1.grad, rtol=1e-6, atol=0)
    torch.testing.assert_close(f.grad, f1.grad, rtol=1e-6, atol=0)
    print(f"\nmse_pair grads bit-equal to torch's: c {torch.equal(c.grad, c1.grad)}, f {torch.equal(f.grad, f1.grad)}")
