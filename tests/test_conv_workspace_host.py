"""Workspace sizes are behaviour: callers allocate by ms_conv1d_workspace_bytes / ms_convt1d_workspace_bytes and the split-K
depth of a row-tile launch follows from the bytes it is given.  tests/golden/conv_workspace.json is the table
(descriptor, pass) -> bytes printed by tools/conv_ws_table.py from a build of the commit BEFORE the row-tile dispatch became a
plan (see that script for how to regenerate it from a parent build and diff); this build must answer the same, exactly.
Host arithmetic only: no kernel is launched, no GPU is needed."""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (the library shares torch's HIP runtime)
    from featuresynth._ops import lib as L
    if not os.path.exists(L.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "music-synthesis_amd", "csrc")])
    return L


def _table():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "conv_workspace.json")))


def test_workspace_bytes_equal_the_recorded_table(lib):
    L = lib.load()
    rows = _table()
    assert len(rows) >= 400
    wrong = []
    for r in rows:
        if r["op"] == "conv":
            got = L.ms_conv1d_workspace_bytes(lib.ConvDesc(*r["desc"]), r["pass"])
        else:
            got = L.ms_convt1d_workspace_bytes(lib.ConvTDesc(*r["desc"]), r["pass"])
        if got != r["bytes"]:
            wrong.append((r["layer"], r["pass"], got, r["bytes"]))
    assert not wrong, "workspace bytes moved (layer, pass, now, recorded): %s" % wrong[:10]


def test_table_covers_the_grid():
    """The recorded table has every layer of tests/test_gpu_dispatch.py (both batch sizes), the shapes of the memory-contract
    suite and the extra shapes of tools/conv_ws_table.py, three passes each, and split-K slabs and packed weights occur."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import conv_ws_table as T
    finally:
        sys.path.pop(0)
    rows = _table()
    have = {(r["op"], tuple(r["desc"]), r["pass"]) for r in rows}
    for op, name, f in T.grid():
        for which in (0, 1, 2):
            assert (op, tuple(f), which) in have, (op, name, which)
    assert len(have) == len(rows)
    layers = {r["layer"] for r in rows}
    for must in ("atom128.d3.B32", "atom32.d9.B1", "d.main5.L4097.B32", "g.convT256.B1", "mc.k5_l17_pad4", "mc.s2_small",
                 "wn.shortcut_c128_b32", "wn.first_k7_reflect", "s1.lines_t_c256_l16", "s1.lines_k3_c256_l16"):
        assert must in layers, must
    assert sum(1 for r in rows if r["bytes"] > 0) >= 200
