"""CPU: the C-ABI library loads, exports every symbol include/nerf_amd.h declares, and its
host-side size helpers agree with the layout (no kernel launches: no GPU here)."""
import os
import re

import pytest

from march_support import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_amd.h")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(nerf_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_hot_path():
    names = declared_functions()
    for must in ("nerf_raygen", "nerf_sample_stratified", "nerf_sample_pdf", "nerf_composite_fwd",
                 "nerf_composite_bwd", "nerf_mlp_fwd", "nerf_mlp_bwd", "nerf_grid_index", "nerf_bake_points",
                 "nerf_march_gather", "nerf_adam_step", "nerf_searchsorted"):
        assert must in names


def test_every_declared_symbol_is_exported(lib):
    from nerf_amd import _lib
    for name in declared_functions():
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature"


def declared_prototypes():
    """name -> (return type, [parameter types]) of every prototype in the header, as C text
    without the parameter names."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(nerf_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = [p.strip() for p in params.split(",")]
        if params == ["void"] or params == [""]:
            params = []
        # drop the parameter's name: what is left of the last identifier, stars kept with the type
        protos[name] = (" ".join(ret.split()), [re.sub(r"\s*\b\w+$", "", p).replace(" *", "*") for p in params])
    return protos


def test_ctypes_signatures_match_the_header():
    """Every prototype of include/nerf_amd.h against _lib.SIGNATURES: the return type, the
    parameter count and each parameter's class (pointer or hipStream_t -> c_void_p, int -> c_int,
    int64_t -> c_int64, uint64_t -> c_uint64, float -> c_float, double -> c_double).  A wrong
    entry would pass garbage to a kernel without any error; nothing is launched here."""
    import ctypes
    from nerf_amd import _lib
    scalars = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
               "double": ctypes.c_double, "hipStream_t": ctypes.c_void_p}

    def ctype_of(c_type, ret=False):
        if c_type.endswith("*"):
            return ctypes.c_char_p if ret and c_type == "const char*" else ctypes.c_void_p
        return scalars[c_type]  # (KeyError: a C type this test does not know yet)

    protos = declared_prototypes()
    assert sorted(protos) == declared_functions() == sorted(_lib.SIGNATURES)
    for name, (ret, params) in protos.items():
        res, args = _lib.SIGNATURES[name]
        assert res is ctype_of(ret, ret=True), f"{name}: returns {ret}, bound as {res}"
        assert len(args) == len(params), f"{name}: {len(params)} parameters declared, {len(args)} bound"
        for i, (p, got) in enumerate(zip(params, args)):
            assert got is ctype_of(p), f"{name}: parameter {i} is {p}, bound as {got}"


def test_sizes_and_layout(lib):
    assert lib.nerf_abi_version() == 4
    assert lib.nerf_mlp_net_params() == 595844
    # state_dict offsets: pts_linears.0.weight [256,63] then bias [256], ... rgb_linear.bias [3]
    assert lib.nerf_mlp_param_offset(0) == 0
    assert lib.nerf_mlp_param_offset(1) == 256 * 63
    assert lib.nerf_mlp_param_offset(24) == 595844
    assert lib.nerf_mlp_padded_samples(1) == 256
    assert lib.nerf_mlp_padded_samples(786432) == 786432
    assert lib.nerf_mlp_act_bytes(1, 256) == 2528 * 256 * 2
    assert lib.nerf_mlp_packed_bytes(1, 0) > 1185000 * 1 and lib.nerf_mlp_packed_bytes(0, 0) > 2 * 1185000
    assert lib.nerf_bake_num_points(128, 1) == 129 ** 3
    assert lib.nerf_bake_num_points(128, 0) == 128 ** 3 * 8


def test_argument_errors_are_reported_without_gpu(lib):
    from nerf_amd._lib import check
    with pytest.raises(RuntimeError, match="dtype"):
        check(lib.nerf_mlp_fwd(None, 7, None, None, 1, None, 10, 0, None, None, None, None), "nerf_mlp_fwd")
    with pytest.raises(RuntimeError, match="Sc"):
        check(lib.nerf_sample_pdf(None, None, 4, 65, 128, 1, None, None, 0, 0, None, None, None, None, None, None,
                                  None), "nerf_sample_pdf")


def test_product_path_rejects_cpu_tensors():
    import torch
    from nerf_amd import ops
    with pytest.raises(RuntimeError, match="GPU only"):
        ops.sample_stratified(torch.zeros(4, 6), 2.0, 6.0, 64, False)


def test_product_path_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "nerf-replication_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), os.path.join(dirpath, f)


def test_bf16x3f_dtype_maps_to_its_parts(lib):
    """NERF_DTYPE_BF16X3F (3): forward pack = bf16x3's, backward pack / stores = bf16's
    (nerf_amd.h: "Every function maps 3 to its part")."""
    text = open(HEADER).read()
    codes = dict(re.findall(r"#define (NERF_DTYPE_\w+) (\d+)", text))
    assert codes == {"NERF_DTYPE_F32": "0", "NERF_DTYPE_BF16": "1", "NERF_DTYPE_BF16X3": "2", "NERF_DTYPE_BF16X3F": "3",
                     "NERF_DTYPE_BF16X6": "4"}
    assert lib.nerf_mlp_packed_bytes(3, 0) == lib.nerf_mlp_packed_bytes(2, 0)
    assert lib.nerf_mlp_packed_bytes(3, 1) == lib.nerf_mlp_packed_bytes(1, 1)
    for M in (1, 4097, 786432):
        assert lib.nerf_mlp_act_bytes(3, M) == lib.nerf_mlp_act_bytes(1, M) == lib.nerf_mlp_act_bytes(2, M) // 2
        assert lib.nerf_mlp_dz_bytes(3, M) == lib.nerf_mlp_dz_bytes(1, M)


def test_packed_layout_sizes(lib):
    """The packed weight layouts (mlp_tables.h): forward 32-row units (fp32 4 KiB / bf16 2 KiB per input tile + a
    bias chunk per unit; 592 tiles, 78 units), the wide bf16x3 forward's 16-row units (2 KiB per K-block + a bias
    chunk; 1,172 K-blocks, 154 units), the 32x32 dX's W^T units (556 tiles) and the wide dX's 16-row W^T units (1,112
    K-blocks, 2 KiB each: the same bytes as fp32's 32-row pack) -- fp32 and bf16x3 run the wide dX, bf16 the 32x32 one."""
    K = 1024
    assert lib.nerf_mlp_packed_bytes(0, 0) == (592 * 4 + 78) * K  # (PF32: the training forward too, NERF_F32_WIDE=0)
    assert lib.nerf_mlp_packed_bytes(1, 0) == (592 * 2 + 78) * K
    assert lib.nerf_mlp_packed_bytes(2, 0) == (1172 * 2 + 154) * K
    assert lib.nerf_mlp_packed_bytes(0, 1) == lib.nerf_mlp_packed_bytes(2, 1) == 1112 * 2 * K == 556 * 4 * K
    assert lib.nerf_mlp_packed_bytes(1, 1) == 556 * 2 * K


def test_bf16x6_is_an_inference_forward_only(lib):
    """NERF_DTYPE_BF16X6 (4): a forward pack and an inference forward; no backward pack, no training
    stores, no backward, no device-count forward."""
    import ctypes
    from nerf_amd._lib import check
    # six 1 KiB chunks per 32-feature input tile (hi, mid, lo of each K half) against fp32's four, + the bias chunks
    p4, p0, p1 = (lib.nerf_mlp_packed_bytes(d, 0) for d in (4, 0, 1))
    assert p4 % 1024 == 0 and p4 - p0 == p0 - p1
    assert lib.nerf_mlp_packed_bytes(4, 1) == -1
    assert lib.nerf_mlp_act_bytes(4, 256) == -1 and lib.nerf_mlp_dz_bytes(4, 256) == -1
    params = ctypes.cast((ctypes.c_void_p * 24)(*([None] * 24)), ctypes.c_void_p)
    dummy = ctypes.c_void_p(16)
    with pytest.raises(RuntimeError, match="backward pack"):
        check(lib.nerf_mlp_pack(params, 4, None, dummy, None), "nerf_mlp_pack")
    for flags in (1, 2):
        with pytest.raises(RuntimeError, match="inference forward only"):
            check(lib.nerf_mlp_fwd(None, 4, None, None, 1, None, 10, flags, None, None, None, None), "nerf_mlp_fwd")
    with pytest.raises(RuntimeError, match="dtype"):
        check(lib.nerf_mlp_bwd_dx(None, 4, None, 10, None, None, None), "nerf_mlp_bwd_dx")
    with pytest.raises(RuntimeError, match="dtype"):
        check(lib.nerf_mlp_fwd_count(None, 4, None, None, 1, None, None, 10, None, None), "nerf_mlp_fwd_count")


@pytest.mark.parametrize("dtype", [-1, 5, 7])
def test_bad_dtype_is_rejected_everywhere(lib, dtype):
    """Every MLP entry point refuses a dtype outside 0..3 before touching any pointer (no GPU
    needed: the argument checks run first)."""
    import ctypes
    from nerf_amd._lib import check
    for helper in ("nerf_mlp_act_bytes", "nerf_mlp_dz_bytes"):
        assert getattr(lib, helper)(dtype, 256) == -1, helper
    assert lib.nerf_mlp_packed_bytes(dtype, 0) == -1 and lib.nerf_mlp_packed_bytes(dtype, 1) == -1
    params = ctypes.cast((ctypes.c_void_p * 24)(*([None] * 24)), ctypes.c_void_p)
    calls = {
        "nerf_mlp_pack": lambda: lib.nerf_mlp_pack(params, dtype, None, None, None),
        "nerf_mlp_fwd": lambda: lib.nerf_mlp_fwd(None, dtype, None, None, 1, None, 10, 0, None, None, None, None),
        "nerf_mlp_fwd_count": lambda: lib.nerf_mlp_fwd_count(None, dtype, None, None, 1, None, None, 10, None, None),
        "nerf_mlp_bwd_dx": lambda: lib.nerf_mlp_bwd_dx(None, dtype, None, 10, None, None, None),
        "nerf_mlp_bwd_dw_ws": lambda: lib.nerf_mlp_bwd_dw_ws(dtype, 10, None, None, None, None, None),
        "nerf_mlp_bwd": lambda: lib.nerf_mlp_bwd(None, dtype, None, 10, None, None, None, None, None),
    }
    for name, call in calls.items():
        with pytest.raises(RuntimeError, match="dtype"):
            check(call(), name)


@pytest.mark.gpu
def test_bf16x3f_through_the_c_abi(cuda, seeded_state):
    """nerf_mlp_pack + nerf_mlp_fwd called through the C ABI (ctypes, no torch wrapper) with
    NERF_DTYPE_BF16X3F: raw is bf16x3's bit for bit, the training stores are the bf16 (hi) halves
    of bf16x3's (bf16 layout, half the bytes), the masks are bf16x3's; dtype 4 is refused."""
    import ctypes
    import torch
    from nerf_amd import ops
    from nerf_amd._lib import check, lib as L, ptr, stream_of
    L = L()
    M, spd = 4133, 7
    g = torch.Generator().manual_seed(5)
    pts = (torch.rand(M, 3, generator=g) * 2.6 - 1.3).to(cuda)
    vd = torch.nn.functional.normalize(torch.randn(-(-M // spd), 3, generator=g), dim=-1).to(cuda)
    params = [seeded_state[f"model.{n}"].to(cuda) for n in ops.NET_PARAM_NAMES]
    arr = ctypes.cast((ctypes.c_void_p * 24)(*[p.data_ptr() for p in params]), ctypes.c_void_p)
    s = stream_of(pts)
    out = {}
    for code in (2, 3):
        fwd = torch.empty(L.nerf_mlp_packed_bytes(code, 0), dtype=torch.uint8, device=cuda)
        bwd = torch.empty(L.nerf_mlp_packed_bytes(code, 1), dtype=torch.uint8, device=cuda)
        check(L.nerf_mlp_pack(arr, code, ptr(fwd), ptr(bwd), s), "pack")
        act = torch.zeros(L.nerf_mlp_act_bytes(code, M), dtype=torch.uint8, device=cuda)
        masks = torch.zeros(L.nerf_mlp_mask_bytes(M), dtype=torch.uint8, device=cuda)
        raw = torch.empty(M, 4, device=cuda)
        check(L.nerf_mlp_fwd(ptr(fwd), code, ptr(pts), ptr(vd), spd, None, M, 1, ptr(raw), ptr(act), ptr(masks), s),
              "fwd")
        out[code] = (fwd, bwd, raw, act, masks)
    torch.cuda.synchronize()
    assert torch.equal(out[2][0], out[3][0])  # forward pack: bf16x3's
    assert out[3][1].numel() == L.nerf_mlp_packed_bytes(1, 1)
    assert torch.equal(out[2][2], out[3][2])  # raw bit for bit
    assert torch.equal(out[2][4], out[3][4])  # ReLU masks
    # bf16x3 tile-block = hi (2 KiB) then lo (2 KiB); bf16x3f keeps the hi 2 KiB of each
    hi = out[2][3].view(-1, 4096)[:, :2048].reshape(-1)
    assert torch.equal(hi, out[3][3])
    raw = torch.empty(M, 4, device=cuda)
    with pytest.raises(RuntimeError, match="dtype"):
        check(L.nerf_mlp_fwd(ptr(out[3][0]), 5, ptr(pts), ptr(vd), spd, None, M, 0, ptr(raw), None, None, s), "fwd")
