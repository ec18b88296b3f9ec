#!/usr/bin/env python3
"""Compare the gfx950 device code of every MLP translation unit between two trees.

    tools/isa_diff.py PARENT_TREE NEW_TREE [--work DIR] [--jobs N] [--reuse-a] [--units REGEX]

For each mlp object the Makefile builds (mlp_abi.o and every mlp_p<prec>_<part>.o) the Makefile's own hipcc
line is taken from `make -n -B`, with `-c mlp.hip -o x.o` replaced by `--cuda-device-only -S -o x.s`, and run
in both trees. The `__hip_cuid_<hash>` symbol is replaced by a fixed token and the pairs are compared: first
as whole files, then, where those differ, per kernel symbol (the instructions, with function-index labels
normalised and assembler comments dropped, plus the .amdhsa_kernel block: registers, LDS, scratch). Exit status
0 only if every kernel is identical and the sets of symbols are equal. A source refactor that must not change the machine code is checked with this."""
import argparse
import concurrent.futures as cf
import os
import re
import subprocess
import sys
import tempfile


def unit_commands(tree):
    """{unit name: hipcc argv that writes the unit's device assembly to '{out}'} from the tree's Makefile."""
    csrc = os.path.join(tree, "nerf-replication_amd", "csrc")
    dry = subprocess.run(["make", "-n", "-B", "-C", csrc, "BUILD=B"], check=True, capture_output=True, text=True)
    cmds = {}
    for line in dry.stdout.splitlines():
        m = re.search(r"^(.*) -c mlp\.hip -o B/(mlp_\w+)\.o$", line.strip())
        if m:
            cmds[m.group(2)] = (csrc, m.group(1).split() + ["--cuda-device-only", "-S", "mlp.hip", "-o"])
    return cmds


def emit(cmd, out, reuse=False):
    """The unit's device assembly (compiled to `out`, or read from it where `reuse`), the cuid symbol masked."""
    if not (reuse and os.path.exists(out)):
        subprocess.run(cmd[1] + [out], cwd=cmd[0], check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", f.read())


def kernels(asm):
    """{symbol: normalised body + kernel descriptor} for every function in one assembly file.  Normalised: the
    function index of the labels dropped, and the assembler comments (no instruction: e.g. the compiler's note of
    which register an undefined value got)."""
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", asm, re.M | re.S):
        body = re.sub(r"[ \t]*;[^\n]*", "", re.sub(r"\.LBB\d+_", ".LBB_", m.group(2)))
        out[m.group(1)] = re.sub(r"\n+", "\n", body)
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\n(.*?)\.end_amdhsa_kernel", asm, re.M | re.S):
        out[m.group(1)] = out.get(m.group(1), "") + m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a"), ap.add_argument("b")
    ap.add_argument("--work", default=None, help="directory for the .s files (default: a temporary one)")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--reuse-a", action="store_true", help="reuse tree A's .s files already under --work")
    ap.add_argument("--units", default="", help="regular expression: only the units it matches (default: all)")
    args = ap.parse_args()
    work = args.work or tempfile.mkdtemp(prefix="isa_diff_")
    ca, cb = ({u: c for u, c in unit_commands(t).items() if re.search(args.units, u)} for t in (args.a, args.b))
    if sorted(ca) != sorted(cb):
        sys.exit(f"unit lists differ: {sorted(set(ca) ^ set(cb))}")
    for side in "ab":
        os.makedirs(os.path.join(work, side), exist_ok=True)
    with cf.ThreadPoolExecutor(args.jobs) as ex:
        fut = {}
        for u in sorted(ca):
            fut["a", u] = ex.submit(emit, ca[u], os.path.join(work, "a", u + ".s"), args.reuse_a)
            fut["b", u] = ex.submit(emit, cb[u], os.path.join(work, "b", u + ".s"))
        bad = 0
        for u in sorted(ca):
            sa, sb = fut["a", u].result(), fut["b", u].result()
            ka, kb = kernels(sa), kernels(sb)
            if sa == sb:
                print(f"{u}: identical ({len(sa.splitlines())} lines, {len(ka)} functions)")
                continue
            diff = sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
            only = sorted(set(ka) ^ set(kb))
            ok = not diff and not only
            bad += not ok
            print(f"{u}: {'identical per kernel (comments or function order differ)' if ok else 'DIFFERENT'} "
                  f"({len(ka)} functions)")
            for k in diff:
                print(f"    differs: {k}")
            for k in only:
                print(f"    only in {'A' if k in ka else 'B'}: {k}")
    print(f"{len(ca)} units, {bad} different")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
