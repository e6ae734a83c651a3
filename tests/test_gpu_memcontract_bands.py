"""Memory contract of the band entries (include/msynth_bands.h), straight through ctypes on tests/memcheck.py's guarded
arena, as tests/test_gpu_memcontract.py does for msynth.h: guard bands around every buffer, outputs and workspace
poisoned twice (NaN pattern, 1e30) with bitwise-equal results, inputs unchanged, a band buffer at an address that is
4-byte but not 16-byte aligned, null band pointers on the two backward entries, and refused calls that must write nothing.
Values are held against the float64 restatement (tests/bands_ref.py) at tests/test_gpu_bands.py's gate.
tests/test_bands_host.py checks that no compute entry is left out."""
import ctypes

import numpy as np
import pytest

import bands_ref as R
from conftest import rel_l2, stable_seed
from memcheck import Arena, GUARD_BYTES, MS_ERR_INVALID_ARG, MS_ERR_UNSUPPORTED, MS_OK

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE = 8.0              # x the float32 stock-FFT error (tests/test_gpu_bands.py)
WS_BYTES = 256          # the entries need no workspace today: a poisoned one is handed over all the same


class Case:
    def __init__(self, id, symbols, fn, args):
        self.id, self.symbols, self.fn, self.args = id, tuple(symbols), fn, args


CASES = []


def case(id, symbols, fn, *args):
    CASES.append(Case(id, [symbols] if isinstance(symbols, str) else symbols, fn, args))


def _L():
    from featuresynth._ops import lib as L
    return L, L.load()


def sync():
    torch.cuda.synchronize()


def rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(stable_seed(seed)).standard_normal(shape).astype(np.float32))


def arena(nfloats, nbuf=24):
    return Arena("cuda", 4 * int(nfloats) + nbuf * (2 * GUARD_BYTES + 1024) + (1 << 20))


def desc(L, sizes, bufs, lowest=1):
    d = L.BandDesc()
    d.count, d.lowest = len(sizes), lowest
    for i, (s, b) in enumerate(zip(sizes, bufs)):
        d.size[i] = s
        d.data[i] = None if b is None else b.ptr
    return d


def held(got, want64, ref32, what):
    e, e32 = rel_l2(got.cpu().numpy(), want64.numpy()), rel_l2(ref32.numpy(), want64.numpy())
    assert e <= GATE * e32, "%s: %.3e against the float64 restatement, stock float32 %.3e" % (what, e, e32)


def split_case(rows, n, m, odd_band, refuse_n):
    """ms_band_decompose_fwd and its adjoint; band `odd_band` sits 4 bytes past a 256-byte boundary."""
    L, lib = _L()
    s = L.stream()
    sizes = R.band_sizes(n, m)
    x = rnd("bx%d%d" % (n, m), rows, 1, n)
    g = [rnd("bg%d%d" % (n, S), rows, 1, S) for S in sizes]
    a = arena(3 * rows * n)
    xb = a.put(x.view(rows, n), name="x")
    outs = [a.take((rows, S), "output", offset_bytes=4 if i == odd_band else 0, name="band%d" % S) for i, S in enumerate(sizes)]
    ws = a.take(max(WS_BYTES, lib.ms_band_workspace_bytes(rows, n, desc(L, sizes, outs))), "workspace", name="ws")
    d = desc(L, sizes, outs)
    rc, out = a.run_twice(lambda: lib.ms_band_decompose_fwd(xb.ptr, rows, n, ctypes.byref(d), ws.ptr, ws.nbytes, s), sync)
    assert rc == MS_OK
    want, ref32 = R.decompose(x.double(), m), R.decompose(x, m)
    for S in sizes:
        held(out["band%d" % S].view(rows, 1, S), want[S], ref32[S], "split band %d" % S)
    bad = L.BandDesc()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(d), ctypes.sizeof(d))
    rc, _ = a.run_twice(lambda: lib.ms_band_decompose_fwd(xb.ptr, rows, refuse_n, ctypes.byref(bad), ws.ptr, ws.nbytes, s), sync)
    assert rc == MS_ERR_UNSUPPORTED
    # the adjoint, every cotangent given
    a2 = arena(3 * rows * n)
    gbs = [a2.put(t.view(rows, S), offset_bytes=4 if i == odd_band else 0, name="g%d" % S) for i, (t, S) in enumerate(zip(g, sizes))]
    gx = a2.take((rows, n), "output", name="grad_x")
    ws2 = a2.take(WS_BYTES, "workspace", name="ws")
    d2 = desc(L, sizes, gbs)
    rc, out = a2.run_twice(lambda: lib.ms_band_decompose_bwd(ctypes.byref(d2), rows, n, gx.ptr, ws2.ptr, ws2.nbytes, s), sync)
    assert rc == MS_OK
    held(out["grad_x"].view(rows, 1, n), R.decompose_adjoint({S: t.double() for S, t in zip(sizes, g)}, n, m),
         R.decompose_adjoint(dict(zip(sizes, g)), n, m), "split adjoint")


def merge_case(rows, sizes, n, odd_band, lowest):
    """ms_band_recompose_fwd and its adjoint."""
    L, lib = _L()
    s = L.stream()
    bands = [rnd("mb%d%d" % (n, S), rows, 1, S) for S in sizes]
    gy = rnd("mg%d" % n, rows, 1, n)
    a = arena(3 * rows * n)
    bbs = [a.put(t.view(rows, S), offset_bytes=4 if i == odd_band else 0, name="band%d" % S) for i, (t, S) in enumerate(zip(bands, sizes))]
    y = a.take((rows, n), "output", offset_bytes=8, name="y")
    ws = a.take(WS_BYTES, "workspace", name="ws")
    d = desc(L, sizes, bbs, lowest)
    rc, out = a.run_twice(lambda: lib.ms_band_recompose_fwd(ctypes.byref(d), rows, n, y.ptr, ws.ptr, ws.nbytes, s), sync)
    assert rc == MS_OK

    def ref(ts):
        if len(sizes) == 1:
            return R.resample(ts[0], n, bool(lowest))
        return R.recompose(dict(zip(sizes, ts)), n)
    held(out["y"].view(rows, 1, n), ref([t.double() for t in bands]), ref(bands), "merge")
    a2 = arena(3 * rows * n)
    gyb = a2.put(gy.view(rows, n), offset_bytes=4, name="grad_y")
    gbs = [a2.take((rows, S), "output", offset_bytes=4 if i == odd_band else 0, name="g%d" % S) for i, S in enumerate(sizes)]
    ws2 = a2.take(WS_BYTES, "workspace", name="ws")
    d2 = desc(L, sizes, gbs, lowest)
    rc, out = a2.run_twice(lambda: lib.ms_band_recompose_bwd(gyb.ptr, rows, n, ctypes.byref(d2), ws2.ptr, ws2.nbytes, s), sync)
    assert rc == MS_OK

    def adj(t):
        if len(sizes) == 1:
            return {sizes[0]: R.resample_adjoint(t, sizes[0], bool(lowest))}
        return R.recompose_adjoint(t, sizes, n)
    want, ref32 = adj(gy.double()), adj(gy)
    for S in sizes:
        held(out["g%d" % S].view(rows, 1, S), want[S], ref32[S], "merge adjoint band %d" % S)


def null_case(rows, n, m, live):
    """Backward entries with null band pointers: only band `live` carries a cotangent / wants a gradient; the buffers of
    the others are in the arena all the same and must stay untouched."""
    L, lib = _L()
    s = L.stream()
    sizes = R.band_sizes(n, m)
    S = sizes[live]
    g = rnd("ng%d%d" % (n, S), rows, 1, S)
    a = arena(3 * rows * n)
    gb = a.put(g.view(rows, S), name="g")
    gx = a.take((rows, n), "output", name="grad_x")
    ws = a.take(WS_BYTES, "workspace", name="ws")
    d = desc(L, sizes, [gb if i == live else None for i in range(len(sizes))])
    rc, out = a.run_twice(lambda: lib.ms_band_decompose_bwd(ctypes.byref(d), rows, n, gx.ptr, ws.ptr, ws.nbytes, s), sync)
    assert rc == MS_OK
    held(out["grad_x"].view(rows, 1, n), R.decompose_adjoint({S: g.double()}, n, m), R.decompose_adjoint({S: g}, n, m),
         "split adjoint of band %d alone" % S)
    gy = rnd("ny%d" % n, rows, 1, n)
    a2 = arena(3 * rows * n)
    gyb = a2.put(gy.view(rows, n), name="grad_y")
    wanted = a2.take((rows, S), "output", name="wanted")
    others = [a2.take((rows, T), "output", name="unwanted%d" % T) for T in sizes if T != S]
    ws2 = a2.take(WS_BYTES, "workspace", name="ws")
    d2 = desc(L, sizes, [wanted if i == live else None for i in range(len(sizes))])
    for poison in ("nan", "big"):
        a2.arm(poison)
        assert lib.ms_band_recompose_bwd(gyb.ptr, rows, n, ctypes.byref(d2), ws2.ptr, ws2.nbytes, s) == MS_OK
        sync()
        assert a2.unwritten(wanted) == 0
        for b in others:
            assert a2.unwritten(b) == b.nbytes // 4, b.name
        assert not [p for p in a2.problems(written=None)]
        got = wanted.t.clone()
    held(got.view(rows, 1, S), R.recompose_adjoint(gy.double(), sizes, n)[S], R.recompose_adjoint(gy, sizes, n)[S],
         "merge adjoint, band %d alone" % S)


def refused_case():
    """Every compute entry, asked for what the kernels do not take: a status, and not one element written."""
    L, lib = _L()
    s = L.stream()
    rows = 2
    a = arena(8 * rows * 128)
    x = a.put(rnd("rx", rows, 96), name="x")
    b16, b32 = a.put(rnd("r16", rows, 16), name="b16"), a.put(rnd("r32", rows, 32), name="b32")
    o8, o16, o32 = (a.take((rows, S), "output", name="o%d" % S) for S in (8, 16, 32))
    y = a.take((rows, 96), "output", name="y")
    ws = a.take(WS_BYTES, "workspace", name="ws")
    calls = [
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_decompose_fwd(x.ptr, rows, 96, ctypes.byref(desc(L, [16, 32], [o16, o32])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_decompose_fwd(x.ptr, rows, 64, ctypes.byref(desc(L, [8, 16], [o8, o16])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_INVALID_ARG, lambda: lib.ms_band_decompose_fwd(x.ptr, rows, 64, ctypes.byref(desc(L, [32, 16], [o32, o16])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_INVALID_ARG, lambda: lib.ms_band_decompose_fwd(x.ptr, rows, 64, ctypes.byref(desc(L, [16, 32], [o16, None])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_decompose_bwd(ctypes.byref(desc(L, [16, 32], [b16, b32])), rows, 96, y.ptr, ws.ptr, ws.nbytes, s)),
        (MS_ERR_INVALID_ARG, lambda: lib.ms_band_decompose_bwd(ctypes.byref(desc(L, [16, 32], [None, None])), rows, 64, y.ptr, ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_recompose_fwd(ctypes.byref(desc(L, [16, 32], [b16, b32])), rows, 96, y.ptr, ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_recompose_fwd(ctypes.byref(desc(L, [16, 32], [b16, b32])), rows, 16, y.ptr, ws.ptr, ws.nbytes, s)),
        (MS_ERR_INVALID_ARG, lambda: lib.ms_band_recompose_fwd(ctypes.byref(desc(L, [16, 32], [b16, None])), rows, 64, y.ptr, ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_recompose_bwd(x.ptr, rows, 96, ctypes.byref(desc(L, [16, 32], [o16, o32])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_UNSUPPORTED, lambda: lib.ms_band_recompose_bwd(x.ptr, rows, 64, ctypes.byref(desc(L, [8, 16], [o8, o16])), ws.ptr, ws.nbytes, s)),
        (MS_ERR_INVALID_ARG, lambda: lib.ms_band_recompose_bwd(x.ptr, 0, 64, ctypes.byref(desc(L, [16, 32], [o16, o32])), ws.ptr, ws.nbytes, s)),
    ]
    for want, call in calls:
        rc, _ = a.run_twice(call, sync)             # verify(written=False): outputs still hold the poison
        assert rc == want, (rc, want)


_SPLIT = ("ms_band_decompose_fwd", "ms_band_decompose_bwd")
_MERGE = ("ms_band_recompose_fwd", "ms_band_recompose_bwd")
case("split_n256_m16_rows6_band2_plus4", _SPLIT, split_case, 6, 256, 16, 2, 96)
case("split_n64_single_band_plus4", _SPLIT, split_case, 3, 64, 64, 0, 32)
case("split_n8192_m512_band4_plus4", _SPLIT, split_case, 2, 8192, 512, 4, 8192 * 8)
case("merge_n256_rows6_band1_plus4", _MERGE, merge_case, 6, [16, 32, 64, 128, 256], 256, 1, 1)
case("merge_up_n1024_missing_band_plus4", _MERGE, merge_case, 3, [64, 256], 1024, 0, 1)
case("merge_resample_not_lowest_plus4", _MERGE, merge_case, 3, [64], 256, 0, 0)
case("merge_n32768_m2048", _MERGE, merge_case, 1, [2048, 4096, 8192, 16384, 32768], 32768, 3, 1)
case("null_gradients_n256_band2", ("ms_band_decompose_bwd", "ms_band_recompose_bwd"), null_case, 3, 256, 16, 2)
case("null_gradients_n8192_band0", ("ms_band_decompose_bwd", "ms_band_recompose_bwd"), null_case, 2, 8192, 512, 0)
case("refused_calls_write_nothing", _SPLIT + _MERGE, refused_case)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_memory_contract(c):
    c.fn(*c.args)
