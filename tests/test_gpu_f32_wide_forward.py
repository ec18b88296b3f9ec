"""The wide fp32 training forward (PF32W, v_mfma_f32_16x16x4_f32, csrc/mlp.hip) against the 32x32x2 one (PF32).

Both f32 MFMA forms are a k-ordered fmaf chain, and the wide kernel feeds the matrix pipe PF32's K sequence
(mlp_tables.h f32w_feat), from PF32's own forward pack.  So the two kernels must agree bit for bit: raw, every
stored activation, every ReLU mask bit.  nerf_mlp_fwd(dtype 0, flags 1) is the default training forward,
flags 1 | 4 (NERF_MLP_F32_NARROW) the 32x32x2 one on the same pack.

Sample counts: 1 and 17 (inside / across a 16-sample wave), 131 (across a 128-sample workgroup), 4099 (several
workgroups and a padded last block).  samples_per_dir 7 (the view direction changes inside a wave) and 192 (it
does not).  Two weight sets: the seed-0 network, and one with every hidden bias set to minus its layer's mean
pre-activation, so that the pre-activations crowd around zero -- where a different summation order would flip
ReLU branches (round 6's wide forward did, 5.6e-7 of them)."""
import pytest
import torch

from march_support import ops

pytestmark = pytest.mark.gpu

MS = (1, 17, 131, 4099)
SPDS = (7, 192)
WIDE, NARROW = 1, 5  # nerf_mlp_fwd flags: NERF_MLP_STORE, NERF_MLP_STORE | NERF_MLP_F32_NARROW


def _inputs(M, spd):
    g = torch.Generator().manual_seed(1000 * M + spd)
    pts = torch.rand(M, 3, generator=g) * 3 - 1.5
    vd = torch.nn.functional.normalize(torch.randn(-(-M // spd), 3, generator=g), dim=-1)
    return pts, vd


def _centered(state, ops):
    """The seed-0 coarse net with each hidden layer's bias moved by minus the mean of that layer's pre-activations
    over the test's own largest input set (torch, CPU): about half of every layer's units then sit on either side
    of the ReLU, many of them within rounding of zero."""
    from oracle import nerf_oracle as O
    p = {n: state[f"model.{n}"].clone() for n in ops.NET_PARAM_NAMES}
    pts, vd = _inputs(4099, 7)
    x = O.positional_encoding(pts, 10)
    d = O.positional_encoding(vd[:, None].expand(-1, 7, 3).reshape(-1, 3)[:4099], 4)
    h = x
    for i in range(8):
        z = torch.nn.functional.linear(h, p[f"pts_linears.{i}.weight"], p[f"pts_linears.{i}.bias"])
        p[f"pts_linears.{i}.bias"] -= z.mean()
        h = torch.relu(z - z.mean())
        if i == 4:
            h = torch.cat([x, h], -1)
    feat = torch.nn.functional.linear(h, p["feature_linear.weight"], p["feature_linear.bias"])
    z = torch.nn.functional.linear(torch.cat([feat, d], -1), p["views_linears.0.weight"], p["views_linears.0.bias"])
    p["views_linears.0.bias"] -= z.mean()
    return [p[n] for n in ops.NET_PARAM_NAMES]


@pytest.fixture(scope="module")
def packs(seeded_state, cuda, ops):
    sets = {"seed0": [seeded_state[f"model.{n}"] for n in ops.NET_PARAM_NAMES], "centered": _centered(seeded_state, ops)}
    return {k: ops.PackedMLP([t.to(cuda).contiguous() for t in v]) for k, v in sets.items()}


def _forward(cuda, pack, M, spd, flags):
    """raw, act and masks of one launch, as CPU tensors (the stores zeroed first: padding no kernel writes is equal)"""
    from nerf_amd._lib import check, lib, ptr, stream_of
    L = lib()
    pts, vd = _inputs(M, spd)
    pc, vc = pts.to(cuda), vd.to(cuda)
    raw = torch.zeros(M, 4, device=cuda)
    store = flags & 1
    act = torch.zeros(L.nerf_mlp_act_bytes(0, M), dtype=torch.uint8, device=cuda) if store else None
    masks = torch.zeros(L.nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda) if store else None
    check(L.nerf_mlp_fwd(ptr(pack.get(0, 0)), 0, ptr(pc), ptr(vc), spd, None, M, flags, ptr(raw), ptr(act), ptr(masks),
                         stream_of(pc)), "nerf_mlp_fwd")
    torch.cuda.synchronize()
    return raw.cpu(), (act.cpu() if store else None), (masks.cpu() if store else None)


@pytest.fixture(scope="module")
def runs(cuda, packs):
    """every (weights, M, spd) case once per forward, shared by the tests below"""
    cache = {}

    def get(w, M, spd, flags):
        key = (w, M, spd, flags)
        if key not in cache:
            cache[key] = _forward(cuda, packs[w], M, spd, flags)
        return cache[key]
    return get


@pytest.mark.parametrize("spd", SPDS)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("weights", ["seed0", "centered"])
def test_wide_equals_narrow_bitwise(runs, weights, M, spd):
    """(a) raw, the act buffer and the mask buffer of the default training forward are the 32x32x2 kernel's bytes"""
    raw_w, act_w, msk_w = runs(weights, M, spd, WIDE)
    raw_n, act_n, msk_n = runs(weights, M, spd, NARROW)
    assert torch.equal(raw_w.view(torch.uint8), raw_n.view(torch.uint8))
    assert torch.equal(act_w, act_n)
    assert torch.equal(msk_w, msk_n)
    assert bool(torch.isfinite(raw_w).all()) and float(raw_w.abs().max()) > 0


def test_centered_weights_crowd_zero(runs):
    """the branch-flip case is one: with the centered biases a large share of every hidden layer is cut by the ReLU
    and a large share is not (tiles 3 .. 66 of the act store are h0 .. h7)"""
    _, act, _ = runs("centered", 4099, 7, WIDE)
    v = act.view(torch.float32).reshape(-1, 79, 4, 64, 4)[:, 3:67]
    nblk = 4099 // 32  # whole blocks only (the padded block repeats the last sample)
    for layer in range(8):
        frac = float((v[:nblk, 8 * layer:8 * layer + 8] > 0).float().mean())
        assert 0.2 < frac < 0.8, (layer, frac)


@pytest.mark.parametrize("spd", SPDS)
@pytest.mark.parametrize("M", MS)
def test_training_raw_equals_inference_raw(runs, M, spd):
    """(b) the training forward's raw is the fp32 inference forward's (flags 0, PF32), bit for bit.  (Confirmed first
    on the parent commit's library: PF32's training and inference forwards wrote the same raw at every M and
    samples_per_dir of this file; the narrow arm repeats that here.)"""
    raw_i, _, _ = runs("seed0", M, spd, 0)
    for flags in (WIDE, NARROW):
        raw_t, _, _ = runs("seed0", M, spd, flags)
        assert torch.equal(raw_t.view(torch.uint8), raw_i.view(torch.uint8)), flags


def _mask_bits(masks, act, M):
    """(mask bit, stored value) of every hidden unit of every sample of the whole blocks: the mask store is
    [block][group 0..8][lane 64][4 dwords], tile n of a group in dword n >> 1 at bit 8 (n & 1) + (rho >> 1) +
    16 (rho & 1); the act store [block][tile 79][chunk 4][lane 64][4] holds register rho = 4 chunk + e"""
    nblk = M // 32
    mk = masks.view(torch.int32).reshape(-1, 9, 64, 4)[:nblk]
    v = act.view(torch.float32).reshape(-1, 79, 4, 64, 4)[:nblk]
    for grp in range(9):
        for n in range(8 if grp < 8 else 4):
            tile = (3 + 8 * grp + n) if grp < 8 else 75 + n
            for rho in range(16):
                bit = (mk[:, grp, :, n >> 1] >> (8 * (n & 1) + (rho >> 1) + 16 * (rho & 1))) & 1
                yield bit, v[:, tile, rho >> 2, :, rho & 3]


@pytest.mark.parametrize("weights", ["seed0", "centered"])
def test_mask_bits_are_the_nonzero_activations(runs, weights):
    """(c) every mask bit equals "stored activation non-zero" (h0 .. h7 and the view layer)"""
    M = 4099
    _, act, masks = runs(weights, M, 7, WIDE)
    for bit, val in _mask_bits(masks, act, M):
        assert torch.equal(bit.bool(), val != 0)
    # the view layer's group uses two of its four dwords; the others are zero
    assert int(masks.view(torch.int32).reshape(-1, 9, 64, 4)[:, 8, :, 2:].abs().max()) == 0


def test_two_runs_are_bit_identical(cuda, packs, runs):
    """(c) two runs of one launch write the same bytes at M = 4099"""
    first = runs("centered", 4099, 7, WIDE)
    again = _forward(cuda, packs["centered"], 4099, 7, WIDE)
    for a, b in zip(first, again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_narrow_flag_is_fp32_training_only(cuda, packs):
    """flags bit 2 with another dtype, or without bit 0, is an error (-22), not a silent default"""
    from nerf_amd._lib import lib, ptr, stream_of
    L = lib()
    pts, vd = _inputs(17, 7)
    pc, vc = pts.to(cuda), vd.to(cuda)
    raw = torch.zeros(17, 4, device=cuda)
    act = torch.zeros(L.nerf_mlp_act_bytes(0, 17), dtype=torch.uint8, device=cuda)
    masks = torch.zeros(L.nerf_mlp_mask_bytes(17), dtype=torch.uint8, device=cuda)
    s = stream_of(pc)
    pf = packs["seed0"].get(0, 0)
    assert L.nerf_mlp_fwd(ptr(pf), 0, ptr(pc), ptr(vc), 7, None, 17, 4, ptr(raw), None, None, s) == -22
    assert L.nerf_mlp_fwd(ptr(pf), 1, ptr(pc), ptr(vc), 7, None, 17, 5, ptr(raw), ptr(act), ptr(masks), s) == -22
    assert b"flags bit 2" in L.nerf_last_error()
