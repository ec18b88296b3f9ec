"""The round march with the MLP taken out of the loop: a synthetic scene, an fp64 reference and a round driver.

The round march (csrc/march.hip: nerf_march_init, nerf_march_gather[_shift], nerf_march_composite[_shift|_used],
nerf_march_finish) is the inference path of render_accelerated and pass A of the training march.  Here the raw
value of a gathered point is looked up in a synthetic field[N, S, 4] by (out_ray, out_step), so that the kernels
under test are the march's alone, the shapes are tiny and an exact per-ray reference exists.

Shared by tests/test_march_rounds_cpu.py (the scene holds every edge class; the reference in fp32 torch agrees with
itself in fp64; a plain-Python model of the round loop ends within the driver's round bound) and
tests/test_gpu_march_rounds.py (the kernels against the reference, and bit-invariance under the round structure).
Nothing here comes from the kernels.

  scene      make_scene(): a 32^3 grid (a half-filled ball, an empty slab), 321 rays (two 256-thread blocks: the
             second one full wave and one lane) through it, a t table of 800 steps, a shift per ray, and for
             either walk (the table as it is / shifted) the brute-force occupancy of every step and the field
  reference  reference(): per ray over its occupied steps in order, volume_renderer.py:327-341 in fp64 (or, the
             same loop, in fp32): sigmoid / relu, alpha = 1 - exp(-sigma step |d|), w = T alpha, sums of w c, w,
             w t, T *= 1 - alpha, stop after the first point with T < t_thresh, white background at the end
  leave-out  the fp32 kernel and fp64 can only disagree on the termination step of a ray whose transmittance
             passes within rounding of t_thresh: 1 - alpha has an absolute error of ~6e-8 and, while T >= 1e-4,
             every factor is >= 1e-4, so the chain's relative error stays below ~1e-3 and the crossing factor
             moves T by under 6e-4 of the threshold.  A ray whose fp64 T comes within 1 % of t_thresh (strictly:
             |T - t_thresh| < 0.01 t_thresh, so t_thresh = 0 leaves nothing out -- T < 0 is false in any
             precision) after any composited point is left out of the comparisons against fp64 (`near`), never
             out of a bit-invariance check.  At most MAX_LEFT_OUT rays may be: test_march_rounds_cpu.py.
  model      model_rounds(): the round loop in plain Python on the reference's per-point T -- the quota from
             T < t_split, the k_low growth, the rays served in index order against cap -- for the round count
  driver     run_rounds(): ops._march's loop through ctypes with the field lookup in place of the MLP
"""
import math

import torch

RES = 32
STEP = 0.005
T_THRESH = 1e-4
N_RAYS = 321
# The seed: about 2.5 % of the rays of this scene family pass within 1 % of t_thresh (a class-2 ray's T falls by
# ~0.87 a step, so one in eight of them lands there): seeds 7 .. 13 leave out 8 .. 14 rays on one walk or the
# other, 14 is the first from 7 upward that meets the cap on both (4 and 6).  Chosen on the fp64 reference
# alone -- nothing of the kernels enters.
SEED = 14
MAX_LEFT_OUT = 6  # 2 % of the rays
BBOX = ((-1.5, -1.5, -1.5), (1.5, 1.5, 1.5))  # the lego one

# the round options of ops.march, at its defaults
DEFAULTS = dict(k_schedule=(12, 24, 48, 96, 192, 384, 768), k_low=8, t_split=0.9, k_low_grow=8, cap=None,
                one_pass=True, macro=True)


# --------------------------------------------------------------------------------------
# the scene
# --------------------------------------------------------------------------------------
def _occupancy(scene, shifted):
    """Brute force: every step's point o + t d in fp32 (t = table + shift: one fp32 add), the reference's index
    arithmetic (oracle.grid_indices) -> occupancy [N, S] bool, the points [N, S, 3], the depths [N, S]."""
    from oracle import nerf_oracle as O
    rays, t = scene["rays"], scene["t_table"]
    N = rays.shape[0]
    tt = t[None, :] + scene["t_shift"][:, None] if shifted else t[None, :].expand(N, -1).contiguous()
    assert tt.dtype == torch.float32
    p = rays[:, None, :3] + tt[:, :, None] * rays[:, None, 3:]
    gi = O.grid_indices(p.reshape(-1, 3), bbox=BBOX, res=RES).reshape(N, -1, 3)
    return scene["grid"][gi[..., 0], gi[..., 1], gi[..., 2]], p, tt


def make_scene(seed=SEED):
    g = torch.Generator().manual_seed(seed)
    # grid: half of the cells of a ball of radius 0.33 res, minus a slab (long empty runs, empty macro blocks)
    grid = torch.rand(RES, RES, RES, generator=g) < 0.5
    c = torch.arange(RES, dtype=torch.float32) - RES / 2
    grid &= (c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2) < (0.33 * RES) ** 2
    grid[:, :, :6] = False
    t_table = torch.arange(2.0, 6.0, STEP)
    S = t_table.numel()
    assert S == 800
    # rays: through a point q of the middle of the box at depth t_q, |d| in [0.25, 1.5]; two that miss the box
    n = N_RAYS - 2
    q = torch.rand(n, 3, generator=g) * 1.5 - 0.75
    t_q = 2.5 + 3.0 * torch.rand(n, generator=g)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=-1)
    d = d * (0.25 + 1.25 * torch.rand(n, 1, generator=g))
    d[::7, 0] = 0.0   # axis-aligned components (before o: these rays go through q too)
    d[::11, 1] = 0.0
    o = q - t_q[:, None] * d
    o = torch.cat([o, torch.tensor([[4.0, 4.0, 4.0], [-4.0, 0.3, 0.2]])])
    d = torch.cat([d, torch.tensor([[0.1, 0.2, 0.3], [0.0, 0.5, 0.0]])])
    rays = torch.cat([o, d], 1).float().contiguous()
    t_shift = (torch.rand(N_RAYS, generator=g) * STEP).float()
    assert float(t_shift.max()) < STEP
    # field: rgb logits 2 randn; the sigma logit by ray class r % 5
    base = torch.randn(N_RAYS, S, 4, generator=g)
    base[..., :3] *= 2.0
    cls = torch.arange(N_RAYS) % 5
    base[cls == 0, :, 3] = -base[cls == 0, :, 3].abs()  # never terminates: acc == 0, white rgb exactly 1
    for k, scale in ((1, 400.0), (2, 40.0), (3, 4.0), (4, 120.0)):  # early, middle, no termination; class 4 below
        base[cls == k, :, 3] *= scale
    scene = dict(grid=grid, t_table=t_table, rays=rays, t_shift=t_shift, cls=cls, N=N_RAYS, S=S, walk={}, _ref={})
    for shifted in (False, True):
        occ, pts, tt = _occupancy(scene, shifted)
        count = occ.sum(1)
        cmax = int(count.max())
        # the occupied steps of every ray, in order, padded with S
        order = torch.argsort((~occ).to(torch.int8), dim=1, stable=True)[:, :cmax]
        occ_steps = torch.where(torch.arange(cmax)[None, :] < count[:, None], order, torch.full_like(order, S))
        # class 4 with more than 12 occupied steps: -1 on the first j, 1e4 on the next (alpha rounds to 1 where
        # 1e4 step |d| is large enough, T to exactly 0): the ray terminates on exactly its 12th (even rays,
        # j = 11) or 13th point -- the last point of a K = 12 round or the first of the next
        field = base.clone()
        for r in torch.nonzero((cls == 4) & (count > 12)).flatten().tolist():
            j = 11 if r % 2 == 0 else 12
            field[r, occ_steps[r, :j], 3] = -1.0
            field[r, occ_steps[r, j], 3] = 1e4
        scene["walk"][shifted] = dict(occ=occ, pts=pts, t=tt, count=count, occ_steps=occ_steps, field=field,
                                      # rank[r, s]: the occupied steps of ray r before step s
                                      rank=torch.cat([torch.zeros(N_RAYS, 1, dtype=torch.long),
                                                      torch.cumsum(occ.long(), 1)], 1))
    return scene


# --------------------------------------------------------------------------------------
# the reference
# --------------------------------------------------------------------------------------
def reference(scene, shifted, t_thresh=T_THRESH, white=True, dtype=torch.float64, n_rays=None):
    """-> dict(rgb [N,3], depth, acc, T (final), used (int64: points composited), near (bool: left out of the
    fp64 comparisons), T_hist [N, Cmax]: T after each composited point (nan elsewhere)).  Cached per argument
    set; never modified."""
    key = (shifted, float(t_thresh), bool(white), dtype, n_rays)
    if key in scene["_ref"]:
        return scene["_ref"][key]
    w_ = scene["walk"][shifted]
    N = scene["N"] if n_rays is None else n_rays
    steps, count = w_["occ_steps"][:N], w_["count"][:N]
    cmax = steps.shape[1]
    valid = torch.arange(cmax)[None, :] < count[:, None]
    sc = steps.clamp(max=scene["S"] - 1)
    rows = torch.arange(N)[:, None]
    raw = w_["field"][rows, sc].to(dtype)   # [N, Cmax, 4]
    t = w_["t"][rows, sc].to(dtype)
    d = scene["rays"][:N, 3:].to(dtype)
    dist = torch.tensor(STEP, dtype=dtype) * torch.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    col = torch.sigmoid(raw[..., :3])
    alpha = 1.0 - torch.exp(-torch.relu(raw[..., 3]) * dist[:, None])
    thr = torch.tensor(t_thresh, dtype=dtype)
    T = torch.ones(N, dtype=dtype)
    rgb, depth, acc = torch.zeros(N, 3, dtype=dtype), torch.zeros(N, dtype=dtype), torch.zeros(N, dtype=dtype)
    alive = torch.ones(N, dtype=torch.bool)
    used = torch.zeros(N, dtype=torch.long)
    near = torch.zeros(N, dtype=torch.bool)
    T_hist = torch.full((N, cmax), float("nan"), dtype=dtype)
    for k in range(cmax):
        act = valid[:, k] & alive
        if not bool(act.any()):
            break
        w = T * alpha[:, k]
        rgb = torch.where(act[:, None], rgb + w[:, None] * col[:, k], rgb)
        acc = torch.where(act, acc + w, acc)
        depth = torch.where(act, depth + w * t[:, k], depth)
        T = torch.where(act, T * (1.0 - alpha[:, k]), T)
        T_hist[:, k] = torch.where(act, T, T_hist[:, k])
        used += act
        near |= act & ((T - thr).abs() < 0.01 * thr)
        alive &= ~(act & (T < thr))
    if white:
        rgb = rgb + (1.0 - acc)[:, None]
    out = dict(rgb=rgb, depth=depth, acc=acc, T=T, used=used, near=near, T_hist=T_hist, terminated=~alive)
    scene["_ref"][key] = out
    return out


# --------------------------------------------------------------------------------------
# the round loop: its options per round, its bound, a model of it
# --------------------------------------------------------------------------------------
def resolve(scene, cfg, shifted):
    """A configuration (a dict over DEFAULTS; k_schedule "cstar" = (c*,) of this walk) -> the full option set,
    with cap = None resolved as ops._march does at the default round_bytes."""
    o = dict(DEFAULTS)
    o.update(cfg)
    if o["k_schedule"] == "cstar":
        o["k_schedule"] = (pick_cstar(scene, shifted)[1],)
    N = o.get("n_rays") or scene["N"]
    if o["cap"] is None:
        o["cap"] = max(N * max(o["k_schedule"]), max(o["k_schedule"]))
    return o


def round_quota(rounds, N, k_schedule, k_low, k_low_grow, cap):
    """(K, k_low) of round `rounds`, as ops._march computes them."""
    K = max(1, min(k_schedule[min(rounds, len(k_schedule) - 1)], cap, (2 ** 31 - 1) // max(N, 1)))
    kl = k_low if k_low_grow <= 0 or rounds < k_low_grow else k_low << min(20, rounds - k_low_grow + 1)
    return K, max(1, min(kl, K))


def round_bound(count, k_schedule, k_low, cap):
    """Rounds a correct march cannot exceed: in every round with a live ray the first reservation starts at 0 and
    fits (K <= cap), so some ray either dies or advances by its whole quota (>= k_min occupied steps) or to the
    end of the table; ray r can do that ceil(count_r / k_min) + 1 times.  One more: the round that finds no ray."""
    k_min = max(1, min(k_low, min(k_schedule), cap))
    return int(sum(math.ceil(int(c) / k_min) + 1 for c in count)) + 1


def model_rounds(scene, shifted, *, k_schedule, k_low, t_split, k_low_grow, cap, t_thresh=T_THRESH, n_rays=None,
                 **_):
    """The round loop in plain Python on the fp64 reference's per-point transmittance -> (rounds with live rays,
    points evaluated).  Rays reserve in index order; a ray whose reservation ends past cap waits (its count still
    moves the reservation counter, as the kernel's atomicAdd does)."""
    ref = reference(scene, shifted, t_thresh, True, torch.float64, n_rays)
    N = scene["N"] if n_rays is None else n_rays
    count = scene["walk"][shifted]["count"][:N].tolist()
    used = ref["used"].tolist()
    term = ref["terminated"].tolist()
    T_hist = ref["T_hist"].tolist()
    pos = [0] * N
    live = list(range(N))
    bound = round_bound(count, k_schedule, k_low, cap)
    rounds = evaluated = 0
    while live:
        assert rounds < bound, (rounds, bound)
        K, kl = round_quota(rounds, N, k_schedule, k_low, k_low_grow, cap)
        reserved = 0
        nxt = []
        for r in live:
            T = 1.0 if pos[r] == 0 else T_hist[r][pos[r] - 1]
            quota = kl if T < t_split else K
            cnt = min(quota, count[r] - pos[r])
            exhausted = cnt < quota  # the walk reached the end of the table
            start = reserved
            reserved += cnt
            if reserved > cap:  # waits: keeps its position
                evaluated += max(0, min(cap - start, cnt))
                nxt.append(r)
                continue
            evaluated += cnt
            pos[r] += cnt
            if term[r] and pos[r] >= used[r]:
                continue  # terminated inside this round's points
            if not exhausted:
                nxt.append(r)
        live = nxt
        rounds += 1
    return rounds, evaluated


def pick_cstar(scene, shifted):
    """(r*, c*): a ray that never terminates, whose last occupied step is followed by empty steps to the end of
    the table, with the count nearest the median of such rays (of at least 64).  With k_schedule = (c*,) it
    gathers everything in round one with exhausted == 0 and must end in round two with no point."""
    w = scene["walk"][shifted]
    ref = reference(scene, shifted)
    last = torch.where(w["count"] > 0, w["occ_steps"].gather(1, (w["count"] - 1).clamp(min=0)[:, None])[:, 0],
                       torch.full_like(w["count"], scene["S"]))
    ok = (~ref["terminated"]) & (last < scene["S"] - 1) & (w["count"] >= 64) & ~ref["near"]
    cand = torch.nonzero(ok).flatten()
    med = w["count"][cand].float().median()
    r = int(cand[(w["count"][cand].float() - med).abs().argmin()])
    return r, int(w["count"][r])


# --------------------------------------------------------------------------------------
# the configurations of the bit-invariance check (over DEFAULTS); each must give the default run's bits
# --------------------------------------------------------------------------------------
TIGHT = N_RAYS * 12 // 4  # three quarters of the rays wait in a K = 12 round
CONFIGS = {
    "default": {},
    "k1": dict(k_schedule=(1,)),
    "k5": dict(k_schedule=(5,)),
    "k12": dict(k_schedule=(12,)),
    "kcstar": dict(k_schedule="cstar"),
    "k800": dict(k_schedule=(800,)),
    "k3_7_64": dict(k_schedule=(3, 7, 64)),
    "k_low1": dict(k_low=1, t_split=0.9),
    "all_low": dict(k_low=8, t_split=2.0),
    "none_low": dict(k_low=8, t_split=0.0),
    "grow0": dict(k_low_grow=0),
    "grow2": dict(k_low_grow=2),
    "two_pass": dict(one_pass=False),
    "no_macro": dict(macro=False),
    "tight_k12": dict(k_schedule=(12,), cap=TIGHT),
    "tight_k12_two_pass": dict(k_schedule=(12,), cap=TIGHT, one_pass=False),
    "tight_sched": dict(k_schedule=(12, 24, 48), cap=TIGHT),
    "tight_sched_two_pass": dict(k_schedule=(12, 24, 48), cap=TIGHT, one_pass=False),
    # one ray's quota is all the room there is: a round serves the first ray to reserve and nobody else
    "cap_is_k_65": dict(k_schedule=(48,), cap=48, n_rays=65),
}


# --------------------------------------------------------------------------------------
# the driver (GPU)
# --------------------------------------------------------------------------------------
def _device_scene(scene, dev):
    key = ("dev", str(dev))
    if key not in scene:
        from nerf_amd._lib import lib, ptr, stream_of
        g8 = scene["grid"].to(device=dev, dtype=torch.uint8).contiguous()
        macro = torch.empty(lib().nerf_march_macro_bytes(RES), dtype=torch.uint8, device=dev)
        assert lib().nerf_march_macro(ptr(g8), RES, ptr(macro), stream_of(g8)) == 0
        scene[key] = dict(rays=scene["rays"].to(dev), t_table=scene["t_table"].to(dev), grid=g8, macro=macro,
                          t_shift=scene["t_shift"].to(dev),
                          field={s: scene["walk"][s]["field"].to(dev) for s in (False, True)})
    return scene[key]


def run_rounds(scene, *, k_schedule, k_low, t_split, k_low_grow, cap, one_pass, macro, t_shift, t_thresh, white,
               n_rays=None, snapshots=False, device="cuda:0"):
    """ops._march's loop through ctypes, the field lookup in place of the MLP.  ``t_shift``: march the scene's
    shifted walk (its t_shift array) or the table as it is.  ``n_rays``: the first so many rays alone.  Every
    buffer is sized cap and K <= cap; the loop is a `for` over round_bound(): running out of rounds is an
    AssertionError.  -> the final state, ray_used, consumed, evaluated (the device counter), evaluated_host (the
    sum over rounds of min(counters[0], cap)), rounds (those with live rays) and, with ``snapshots``, per round
    the state entering it, what the gather wrote and the state after the composite -- all on the CPU."""
    from nerf_amd import ops
    from nerf_amd._lib import check, lib, ptr, stream_of
    dev = torch.device(device)
    D = _device_scene(scene, dev)
    L = lib()
    shifted = bool(t_shift)
    N = scene["N"] if n_rays is None else int(n_rays)
    S = scene["S"]
    cap = int(cap)
    assert 1 <= N <= scene["N"] and cap >= 1
    rays = D["rays"][:N].contiguous()
    shift = D["t_shift"][:N].contiguous() if shifted else None
    field = D["field"][shifted]
    t_table, g8 = D["t_table"], D["grid"]
    mg = D["macro"] if macro else None
    f = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=dev)  # noqa: E731
    T, rgb, dep, acc = f(N), f(N, 3), f(N), f(N)
    nxt, off, cnt = (f(N, dt=torch.int32) for _ in range(3))
    start = None if one_pass else f(N, dt=torch.int32)
    alive, exh = f(N, dt=torch.uint8), f(N, dt=torch.uint8)
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    stats = torch.zeros(2, dtype=torch.int64, device=dev)  # [0] consumed, [1] evaluated
    used = torch.zeros(N, dtype=torch.int32, device=dev)
    out_ray, out_step, out_pts, raw = f(cap, dt=torch.int32), f(cap, dt=torch.int32), f(cap, 3), f(cap, 4)
    s = stream_of(rays)
    bb = ops._bbox_arr(BBOX)
    state = (ptr(T), ptr(rgb), ptr(dep), ptr(acc), ptr(nxt), ptr(alive), ptr(exh))
    check(L.nerf_march_init(*state, N, s), "nerf_march_init")
    snaps = []
    cpu = lambda **kw: {k: v.cpu().clone() for k, v in kw.items()}  # noqa: E731
    evaluated_host = live_rounds = 0
    bound = round_bound(scene["walk"][shifted]["count"][:N], k_schedule, k_low, cap)
    for rounds in range(bound):
        K, kl = round_quota(rounds, N, k_schedule, k_low, k_low_grow, cap)
        assert 1 <= kl <= K <= cap
        counters.zero_()
        out_ray.fill_(-1)
        out_step.fill_(-1)
        out_pts.fill_(float("nan"))
        raw.fill_(float("nan"))
        if snapshots:
            snap = dict(K=K, k_low=kl, before=cpu(T=T, next_step=nxt, alive=alive, exhausted=exh, ray_used=used))
        check(L.nerf_march_gather_shift(ptr(rays), N, ptr(t_table), S, ptr(g8), RES, ptr(mg), bb, K, kl,
                                        float(t_split), *state, ptr(counters), stats[1:].data_ptr(), ptr(start),
                                        ptr(out_ray), ptr(out_step), ptr(out_pts), ptr(off), ptr(cnt), cap,
                                        ptr(shift), s), "nerf_march_gather")
        c = counters.tolist()
        n = min(c[0], cap)
        assert n >= 0
        if n > 0:
            ri, si = out_ray[:n].long(), out_step[:n].long()
            assert bool(((ri >= 0) & (ri < N) & (si >= 0) & (si < S)).all()), "gathered ids out of range"
            raw[:n] = field[ri, si]
        if snapshots:
            snap.update(counters=c, n=n, gather=cpu(out_ray=out_ray, out_step=out_step, out_pts=out_pts, ray_off=off,
                                                    ray_cnt=cnt, next_step=nxt, exhausted=exh, alive=alive))
        check(L.nerf_march_composite_shift(ptr(raw), ptr(rays), N, ptr(t_table), ptr(off), ptr(cnt), ptr(out_step),
                                           *state, STEP, float(t_thresh), stats.data_ptr(), ptr(used), ptr(shift), s),
              "nerf_march_composite")
        if snapshots:
            snap["after"] = cpu(T=T, alive=alive, ray_used=used, rgb=rgb, depth=dep, acc=acc)
            snaps.append(snap)
        evaluated_host += n
        if c[1] == 0:
            break
        live_rounds += 1
    else:
        raise AssertionError(f"the march did not end within {bound} rounds")
    check(L.nerf_march_finish(ptr(rgb), ptr(acc), N, int(bool(white)), s), "nerf_march_finish")
    st = stats.tolist()
    out = cpu(rgb=rgb, depth=dep, acc=acc, T=T, alive=alive, exhausted=exh, next_step=nxt, ray_used=used)
    out.update(consumed=int(st[0]), evaluated=int(st[1]), evaluated_host=evaluated_host, rounds=live_rounds,
               bound=bound, snaps=snaps)
    return out
