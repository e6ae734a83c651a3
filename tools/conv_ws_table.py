"""Workspace bytes and kernel name of every conv / transposed-conv pass over a fixed grid of geometries, read from the
library's host-side queries (ms_conv1d_workspace_bytes / _kernel_name and the convt pair; nothing is launched, no GPU).

Workspace sizes are behaviour -- callers allocate by them and the split-K depth follows from them -- so a change that
only moves dispatch code must leave the column as it was.  tests/golden/conv_workspace.json is this table without the
names, and it is made from a build of the commit BEFORE such a change, never from the branch under review:

    git worktree add ../parent <parent commit> && make -C ../parent/music-synthesis_amd/csrc -j16
    MSYNTH_LIB=../parent/music-synthesis_amd/featuresynth/_lib/libmsynth_hip.so python tools/conv_ws_table.py --no-names \
        > tests/golden/conv_workspace.json

tests/test_conv_workspace_host.py holds the branch to it.  With the names (the default) two builds are compared by
diffing the two outputs: one JSON object per line.

The grid: the layers of tests/test_gpu_dispatch.py (both batch sizes), the shapes of the memory-contract suite
(tests/test_gpu_memcontract.py _S / _T), the weight-normed MelGAN's pointwise and reflection-padded k7 convs
(tests/test_gpu_realmelgan.py), and stage-1 lines: the 2-D (transposed) convs run as thousands of rows of 16 .. 64."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "music-synthesis_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

SLOPE = 0.2

# name, B, Cin, L, Cout, K, stride, pad, dil, groups, pad_mode, act, in_act
EXTRA_CONVS = [
    ("wn.shortcut_c32", 3, 32, 1031, 32, 1, 1, 0, 1, 1, 0, 0, 0), ("wn.shortcut_c32_l1024", 3, 32, 1024, 32, 1, 1, 0, 1, 1, 0, 0, 0),
    ("wn.shortcut_c64_l2048", 2, 64, 2048, 64, 1, 1, 0, 1, 1, 0, 0, 0), ("wn.shortcut_c128_l256", 2, 128, 256, 128, 1, 1, 0, 1, 1, 0, 0, 0),
    ("wn.shortcut_c128_l257", 2, 128, 257, 128, 1, 1, 0, 1, 1, 0, 0, 0), ("wn.shortcut_c256_l64", 5, 256, 64, 256, 1, 1, 0, 1, 1, 0, 0, 0),
    ("wn.shortcut_c128_b32", 32, 128, 2048, 128, 1, 1, 0, 1, 1, 0, 0, 0), ("wn.shortcut_c256_b32", 32, 256, 256, 256, 1, 1, 0, 1, 1, 0, 0, 0),
    ("wn.first_k7_reflect", 2, 128, 9, 512, 7, 1, 3, 1, 1, 1, 0, 0), ("wn.first_k7_reflect_b32", 32, 128, 32, 512, 7, 1, 3, 1, 1, 1, 0, 0),
    ("wn.last_k7_reflect_tanh", 2, 32, 515, 1, 7, 1, 3, 1, 1, 1, 2, 1), ("wn.k7_reflect_c64", 4, 64, 300, 64, 7, 1, 3, 1, 1, 1, 1, 0),
    ("wn.k7_reflect_c128_b32", 32, 128, 256, 128, 7, 1, 3, 1, 1, 1, 1, 1),
    ("wn.res_conv3_c64_reflect", 2, 64, 300, 64, 3, 1, 3, 3, 1, 1, 1, 1), ("wn.res_conv3_c256_d9_reflect", 2, 256, 70, 256, 3, 1, 9, 9, 1, 1, 1, 1),
    ("wn.res_conv3_c128_in_act", 32, 128, 2048, 128, 3, 1, 3, 3, 1, 0, 1, 1),
    ("s1.lines_k3_c256_l16", 4096, 256, 16, 256, 3, 1, 1, 1, 1, 0, 1, 0), ("s1.lines_k3_c128_l32", 2048, 128, 32, 128, 3, 1, 1, 1, 1, 0, 1, 0),
    ("s1.lines_k3_c64_l64", 2048, 64, 64, 64, 3, 1, 1, 1, 1, 0, 1, 0), ("s1.lines_k5_c256_l16", 1024, 256, 16, 256, 5, 1, 2, 1, 1, 0, 1, 0),
    ("s1.lines_k3_c512_l16", 1024, 512, 16, 512, 3, 1, 1, 1, 1, 0, 0, 0),
]
# name, B, Cin, L, Cout, K, stride, pad, act, in_act
EXTRA_CONVTS = [
    ("s1.lines_t_c512_l16", 1024, 512, 16, 256, 4, 2, 1, 1, 0), ("s1.lines_t_c256_l16", 4096, 256, 16, 128, 4, 2, 1, 1, 0),
    ("s1.lines_t_c128_l32", 2048, 128, 32, 64, 4, 2, 1, 1, 0), ("s1.lines_t_c64_l64", 2048, 64, 64, 32, 4, 2, 1, 1, 1),
    ("s1.lines_t_c256_l24", 3000, 256, 24, 128, 4, 2, 1, 0, 0), ("s1.lines_t_c128_l64_b1k", 1024, 128, 64, 128, 4, 2, 1, 1, 0),
    ("g.convT_in_act_b32", 32, 512, 32, 256, 16, 8, 4, 1, 1), ("g.convT_s2_in_act_b32", 32, 128, 2048, 64, 4, 2, 1, 1, 1),
]


def grid():
    """-> [("conv" | "convt", name, descriptor fields)], in a fixed order"""
    import test_gpu_dispatch as D
    import test_gpu_memcontract as M
    rows = []
    for c in D.CONVS:
        rows.append(("conv", "%s.B%d" % (c[0], c[1]), tuple(c[1:]) + (SLOPE, 0)))
    for c in D.CONVTS:
        rows.append(("convt", "%s.B%d" % (c[0], c[1]), tuple(c[1:]) + (SLOPE, 0)))
    for key in sorted(M._S):
        name, B, Cin, Lg, Cout, K, st, pad, dil, g, act, refl = M._S[key]
        rows.append(("conv", "mc." + key, (B, Cin, Lg, Cout, K, st, pad, dil, g, 1 if refl else 0, act, SLOPE, 0)))
    for key in sorted(M._T):
        name, B, Cin, Lg, Cout, K, st, pad = M._T[key]
        rows.append(("convt", "mc." + key, (B, Cin, Lg, Cout, K, st, pad, 1, SLOPE, 0)))
    for c in EXTRA_CONVS:
        rows.append(("conv", c[0], tuple(c[1:12]) + (SLOPE, c[12])))
    for c in EXTRA_CONVTS:
        rows.append(("convt", c[0], tuple(c[1:9]) + (SLOPE, c[9])))
    seen = set()        # (a shape two suites share is listed once, under the first name)
    return [r for r in rows if not ((r[0], r[2]) in seen or seen.add((r[0], r[2])))]


def table(names=True):
    from featuresynth._ops import lib as L
    lib = L.load()
    out = []
    for op, name, f in grid():
        d = (L.ConvDesc if op == "conv" else L.ConvTDesc)(*f)
        ws = lib.ms_conv1d_workspace_bytes if op == "conv" else lib.ms_convt1d_workspace_bytes
        kn = lib.ms_conv1d_kernel_name if op == "conv" else lib.ms_convt1d_kernel_name
        for which in (0, 1, 2):
            row = {"op": op, "layer": name, "desc": list(f), "pass": which, "bytes": int(ws(d, which))}
            if names:
                row["kernel"] = kn(d, which).decode()
            out.append(row)
    return out


if __name__ == "__main__":
    rows = table("--no-names" not in sys.argv[1:])
    print("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]")
