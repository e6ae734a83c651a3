"""Band split / merge, the parts that need no GPU: the float64 restatement (tests/bands_ref.py) against the reference's
own float32 outputs (tests/golden/multiscale.npz, written by tools/make_golden_multiscale.py), the hand-written adjoints
against autograd, and the bookkeeping of the band C ABI (include/msynth_bands.h)."""
import ctypes
import os
import re

import numpy as np
import pytest

import bands_ref as R
from conftest import rel_l2

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The reference's float32 output against the float64 restatement measures 1.3e-7 .. 2.2e-7 (split, merge, gradient at
# N = 256, 8192, 32768): float32 rounding of a stock FFT.  1e-6 is about 5x that.
FIXTURE_TOL = 1e-6
CASES = {"a": dict(N=256, m=16, merges=(256, 1024), resample=64), "b": dict(N=2048, m=128, merges=(2048,), resample=512)}


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_matches_the_reference_fixture(golden, name):
    g, c = golden("multiscale"), CASES[name]
    x = torch.from_numpy(g[name + "_x"]).double()
    assert x.shape[-1] == c["N"]
    bands = R.decompose(x, c["m"])
    sizes = R.band_sizes(c["N"], c["m"])
    assert list(bands.keys()) == sizes
    seen = 0
    for S in sizes:
        want = g["%s_band_%d" % (name, S)]
        assert tuple(bands[S].shape) == want.shape == x.shape[:-1] + (S,)
        e = rel_l2(want, bands[S].numpy())
        assert e <= FIXTURE_TOL, (S, e)
        seen += 1
    # the merges and the resamples take the REFERENCE's float32 bands, as the reference did
    ref_bands = {S: torch.from_numpy(g["%s_band_%d" % (name, S)]).double() for S in sizes}
    for D in c["merges"]:
        e = rel_l2(g["%s_merge_%d" % (name, D)], R.recompose(ref_bands, D).numpy())
        assert e <= FIXTURE_TOL, (D, e)
        seen += 1
    for lowest in (True, False):
        want = g["%s_resample_%d_%s" % (name, c["resample"], "lowest" if lowest else "other")]
        e = rel_l2(want, R.resample(ref_bands[c["m"]], c["resample"], lowest).numpy())
        assert e <= FIXTURE_TOL, (lowest, e)
        seen += 1
    assert seen + 1 == len([k for k in g.files if k.startswith(name + "_")])         # every array of the case was held


def test_split_then_merge_is_not_the_identity():
    """Neighbouring bands both carry bin S/2: 2-3 % on noise, in the reference too (the fixture's own arrays)."""
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 1, 8192)))
    e = rel_l2(R.recompose(R.decompose(x, 512), 8192).numpy(), x.numpy())
    assert 0.01 < e < 0.05, e


@pytest.mark.parametrize("N,m", [(64, 64), (256, 16), (2048, 128)])
def test_adjoints_by_hand_match_autograd(N, m):
    rng = np.random.default_rng(N + m)
    sizes = R.band_sizes(N, m)
    x = torch.from_numpy(rng.standard_normal((2, 3, N))).requires_grad_(True)
    g = {S: torch.from_numpy(rng.standard_normal((2, 3, S))) for S in sizes}
    out = R.decompose(x, m)
    dot = sum((out[S] * g[S]).sum() for S in sizes)
    dot.backward()
    gx = R.decompose_adjoint(g, N, m)
    assert rel_l2(gx.numpy(), x.grad.numpy()) <= 1e-13
    assert abs(float((x.detach() * gx).sum()) - float(dot.detach())) <= 1e-12 * abs(float(dot.detach()))          # <A x, g> = <x, A^T g>
    if len(sizes) > 1:          # a band without cotangent
        x.grad = None
        (R.decompose(x, m)[sizes[1]] * g[sizes[1]]).sum().backward()
        assert rel_l2(R.decompose_adjoint({sizes[1]: g[sizes[1]]}, N, m).numpy(), x.grad.numpy()) <= 1e-13
    for D in (N, 4 * N):
        bands = {S: torch.from_numpy(rng.standard_normal((2, 3, S))).requires_grad_(True) for S in sizes}
        gy = torch.from_numpy(rng.standard_normal((2, 3, D)))
        dot = (R.recompose(bands, D) * gy).sum()
        dot.backward()
        gb = R.recompose_adjoint(gy, sizes, D)
        for S in sizes:
            assert rel_l2(gb[S].numpy(), bands[S].grad.numpy()) <= 1e-13, (D, S)
        back = sum(float((bands[S].detach() * gb[S]).sum()) for S in sizes)
        assert abs(back - float(dot.detach())) <= 1e-12 * abs(float(dot.detach()))
    for lowest in (True, False):
        b = torch.from_numpy(rng.standard_normal((2, 3, m))).requires_grad_(True)
        gy = torch.from_numpy(rng.standard_normal((2, 3, 4 * m)))
        (R.resample(b, 4 * m, lowest) * gy).sum().backward()
        assert rel_l2(R.resample_adjoint(gy, m, lowest).numpy(), b.grad.numpy()) <= 1e-13


# ---------------------------------------------------------------- the band C ABI

def declared_band_symbols():
    text = open(os.path.join(ROOT, "include", "msynth_bands.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(ms_[a-z0-9_]+)\s*\(", text))


@pytest.fixture(scope="module")
def lib():
    from featuresynth._ops import lib as L
    if not os.path.exists(L.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "music-synthesis_amd", "csrc")])
    return L


def test_header_table_and_library_name_the_same_symbols(lib):
    declared = declared_band_symbols()
    assert declared == {"ms_band_supported", "ms_band_workspace_bytes", "ms_band_decompose_fwd", "ms_band_decompose_bwd",
                        "ms_band_recompose_fwd", "ms_band_recompose_bwd"}
    assert set(lib.BAND_SIGNATURES) == declared
    assert not set(lib.BAND_SIGNATURES) & set(lib.SIGNATURES)
    # what the library exports: the names of its dynamic string table (kernels are C++-mangled, these are not)
    blob = open(lib.LIB_PATH, "rb").read()
    exported = {m.decode() for m in re.findall(rb"\x00(ms_band_[a-z0-9_]+)(?=\x00)", blob)}
    assert exported == declared, sorted(exported ^ declared)
    raw = ctypes.CDLL(lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    bound = lib.load()
    for name, (res, args) in lib.BAND_SIGNATURES.items():
        fn = getattr(bound, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert ctypes.sizeof(lib.BandDesc) == 8 + lib.BAND_MAX * (4 + 8)                  # ms_band_desc


def test_integration_md_lists_every_band_entry():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in declared_band_symbols():
        assert name in text, name


def _desc(lib, sizes, lowest=1):
    d = lib.BandDesc()
    d.count, d.lowest = len(sizes), lowest
    for i, s in enumerate(sizes):
        d.size[i] = s
    return d


def test_host_side_queries_and_refusals(lib):
    L = lib.load()
    ok = [(64, [64]), (256, [16, 32, 64, 128, 256]), (8192, [512, 1024, 2048, 4096, 8192]), (32768, [2048, 32768]),
          (1024, [64, 256]), (32768, [16 << i for i in range(8)])]
    for n, sizes in ok:
        assert L.ms_band_supported(n, _desc(lib, sizes)) == 1, (n, sizes)
        assert L.ms_band_workspace_bytes(32, n, _desc(lib, sizes)) == 0
    bad = [(96, [16, 32]), (32, [16, 32]), (65536, [4096]), (64, [8, 16]), (256, [16, 48]), (256, [16, 512]),
           (256, [32, 16]), (256, [16, 16]), (256, [])]
    for n, sizes in bad:
        assert L.ms_band_supported(n, _desc(lib, sizes)) == 0, (n, sizes)
    # refused before anything is launched (no device is touched: these run without a GPU)
    d = _desc(lib, [16, 32])
    assert L.ms_band_decompose_fwd(None, 1, 64, d, None, 0, None) == -1                 # null input
    assert L.ms_band_decompose_fwd(0x1000, 1, 96, d, None, 0, None) == -2               # 96 samples
    assert L.ms_band_decompose_fwd(0x1000, 1, 64, d, None, 0, None) == -1               # null band pointers
    assert L.ms_band_recompose_fwd(_desc(lib, [8, 16]), 1, 64, 0x1000, None, 0, None) == -2
    assert L.ms_band_decompose_bwd(d, 1, 64, 0x1000, None, 0, None) == -1               # no cotangent at all
    assert L.ms_band_recompose_bwd(0x1000, 0, 64, d, None, 0, None) == -1               # no rows
    nine = lib.BandDesc()
    nine.count = 9
    assert L.ms_band_recompose_bwd(0x1000, 1, 64, nine, None, 0, None) == -2


EXEMPT = {
    "ms_band_supported": "host-only geometry query",
    "ms_band_workspace_bytes": "host-only size query",
}


def test_every_band_entry_has_a_memory_contract_case(lib):
    import test_gpu_memcontract_bands as T
    named = set()
    for c in T.CASES:
        assert c.symbols, c.id
        named.update(c.symbols)
    assert not (named | set(EXEMPT)) - set(lib.BAND_SIGNATURES)
    assert not named & set(EXEMPT)
    missing = set(lib.BAND_SIGNATURES) - named - set(EXEMPT)
    assert not missing, "band entries without a memory-contract case (tests/test_gpu_memcontract_bands.py): %s" % sorted(missing)
    ids = [c.id for c in T.CASES]
    assert len(ids) == len(set(ids))
    # each compute entry is held by a null-pointer case and by a refused call as well
    for kind in ("null", "refused"):
        covered = set()
        for c in T.CASES:
            if kind in c.id:
                covered.update(c.symbols)
        assert covered >= set(lib.BAND_SIGNATURES) - set(EXEMPT) - ({"ms_band_decompose_fwd", "ms_band_recompose_fwd"}
                                                                    if kind == "null" else set()), (kind, covered)
