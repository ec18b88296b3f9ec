"""The K order of the wide fp32 forward (csrc/mlp_tables.h f32w_feat / f32w_row, csrc/mlp.hip PF32W) on the CPU.

The wide kernel is bit-identical to the 32x32x2 one only if it multiplies the same weight columns in the same
order.  A host program prints the wide forward's own tables; this test rebuilds PF32's sequence from the MFMA
register layout alone and compares:
  * 32x32x2 MFMA rho = 0..15 of input tile t takes feature (rho & 3) + 8 (rho >> 2) of lane half 0, then the
    same + 4 of lane half 1: position 2 rho + h of the tile's K sequence;
  * a 16x16x4 MFMA sums its lane groups g = 0..3 in order: MFMA j of K-block t covers positions 4 j + g;
  * accumulator row 4 g + e of 16-row unit mt is register 4 (mt & 1) + e of lane group g of the next layer's
    K-block mt >> 1, so the weight row it carries must be the feature at position 4 (4 (mt & 1) + e) + g;
  * a lane's two A values of MFMAs 2b, 2b + 1 are the adjacent elements 2 (g >> 1), 2 (g >> 1) + 1 of PF32's
    packed 16-byte slot (chunk b), i.e. one aligned 8-byte read."""
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
MLP = os.path.join(ROOT, "nerf-replication_amd", "csrc", "mlp.hip")

pytestmark = pytest.mark.skipif(shutil.which(HIPCC) is None, reason="no hipcc")

# (input tiles, first weight column of tile t, valid columns of tile t) per forward layer, from the network
# (network.py: xyz encoding 63 wide, skip into layer 5, view encoding 27 wide after the 256 features)
LAYERS = ["L0", "L1", "L2", "L3", "L4", "L5", "L6", "L7", "LFA", "LV", "LRGB"]


def _tiles(layer):
    if layer == "L0":
        return [(0, 32), (32, 31)]
    if layer == "L5":
        return [(0, 32), (32, 31)] + [(63 + 32 * t, 32) for t in range(8)]
    if layer == "LV":
        return [(32 * t, 32) for t in range(8)] + [(256, 27)]
    if layer == "LRGB":
        return [(32 * t, 32) for t in range(4)]
    return [(32 * t, 32) for t in range(8)]


def _pf32_sequence():
    """the 32 features of an input tile in the order the 32x32x2 forward sums them"""
    return [(rho & 3) + 8 * (rho >> 2) + 4 * h for rho in range(16) for h in range(2)]


@pytest.fixture(scope="module")
def tables():
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "order.hip")
        with open(src, "w") as f:
            f.write("#define NERF_MLP_DEVICE_ONLY\n")
            f.write(f'#include "{MLP}"\n#include <cstdio>\nusing namespace nerf::mlp;\nint main() {{\n')
            f.write("  for (int L = 0; L < NLAYER; ++L)\n    for (int t = 0; t < fwd_in_tiles(L); ++t)\n"
                    "      for (int j = 0; j < 8; ++j)\n        for (int g = 0; g < 4; ++g)\n"
                    '          printf("col %d %d %d %d %d\\n", L, t, j, g, f32w_fwd_column(L, t, j, g));\n')
            f.write('  for (int a = 0; a < 16; ++a) printf("row %d %d\\n", a, f32w_row(a));\n')
            f.write("  for (int c = 0; c < 4; ++c)\n    for (int e = 0; e < 4; ++e)\n"
                    '      printf("rho %d %d %d\\n", c, e, PF32::rho_of(c, e));\n')
            f.write("  for (int g = 0; g < 4; ++g)\n    for (int e = 0; e < 8; ++e)\n"
                    '      printf("feat %d %d %d\\n", g, e, PF32W::fwd_feat(g, e));\n')
            f.write("}\n")
        exe = os.path.join(tmp, "order")
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O0", "-std=c++17", "-fconstexpr-steps=33554432",
                        f"-I{ROOT}/include", src, "-o", exe], check=True, capture_output=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    t = {"col": {}, "row": {}, "rho": {}, "feat": {}}
    for line in out:
        kind, *v = line.split()
        v = [int(x) for x in v]
        t[kind][tuple(v[:-1])] = v[-1]
    return t


def test_wide_forward_walks_pf32_sequence(tables):
    seq = _pf32_sequence()
    assert sorted(seq) == list(range(32)) and seq[:8] == [0, 4, 1, 5, 2, 6, 3, 7]
    n = 0
    for L, layer in enumerate(LAYERS):
        for t, (base, valid) in enumerate(_tiles(layer)):
            for j in range(8):
                for g in range(4):
                    f = seq[4 * j + g]
                    assert tables["col"][(L, t, j, g)] == (base + f if f < valid else -1), (layer, t, j, g)
                    n += 1
    assert n == len(tables["col"])  # (every layer and K-block the kernel has, and no other)


def test_pe_registers_follow_the_same_map(tables):
    seq = _pf32_sequence()
    for g in range(4):
        for e in range(8):
            assert tables["feat"][(g, e)] == seq[4 * e + g]


def test_output_rows_land_on_the_next_layers_registers(tables):
    seq = _pf32_sequence()
    rows = [tables["row"][(a,)] for a in range(16)]
    assert sorted(rows) == list(range(16))  # a permutation of the unit's rows
    for mt in range(2):
        for g in range(4):
            for e in range(4):
                assert 16 * mt + rows[4 * g + e] == seq[4 * (4 * mt + e) + g]
    # the scalar outputs: alpha is row 0 (register 0 of lane group 0); rgb rows 0, 1, 2 are A-rows 0, 8, 1
    assert rows[0] == 0 and rows[8] == 1 and rows[1] == 2


def test_packed_slot_pairs_are_adjacent(tables):
    """PF32's packed slot (chunk b) holds rho_of(b, 0..3); lane group g of the wide kernel multiplies register
    2 j + (g >> 1) in MFMA j: for j = 2b, 2b + 1 these are elements 2 (g >> 1) and 2 (g >> 1) + 1 of the slot"""
    for b in range(4):
        assert sorted(tables["rho"][(b, e)] for e in range(4)) == [4 * b + i for i in range(4)]
        for g in range(4):
            for i in range(2):
                assert tables["rho"][(b, 2 * (g >> 1) + i)] == 2 * (2 * b + i) + (g >> 1)
