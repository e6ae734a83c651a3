"""Memory contract of the C ABI (run with -m gpu on an MI355X), straight through ctypes: every buffer of a call is carved out
of one guarded arena (tests/memcheck.py), so the suite sees
  - a store outside an output or outside the queried workspace bytes (guard bands on both sides of every buffer),
  - an input that changed,
  - an output element that was never written (NaN-pattern / 1e30 pre-fill),
  - a result that depends on what scratch or output memory held before the call (run twice under both poisons),
  - what happens when an operand sits at an address that is only 4-byte aligned (handled, or refused with a status),
and the values are compared with the float64 reference of the op's own parity test at that test's tolerance: no new numeric
gate.  Each case names the C-ABI symbols it exists for; tests/test_memcheck_host.py checks that none is left out.

Short workspaces: the ABI has one size query per pass (the largest need over the plan's routes), and for every SHORT_WS route
here the route behind it needs at least as much, so "the next route's size" cannot be passed; those routes are declined with no
workspace instead, which ends in MS_OK where a later route needs none and in MS_ERR_WORKSPACE (nothing written) otherwise.

Routes held to a tolerance instead of bitwise equality between the two poisoned runs (float atomics):
  - k_reflect_fold_bwd (conv_direct.hip): mirrored taps of a reflection-padded conv's backward data meet on one sample
    through atomicAdd when Lin <= 2 pad + 1 (case conv_D_DIRECT_reflect_fold_colliding); compared at GRAD_TOL.  Longer rows are
    held bitwise.
"""
import ctypes

import numpy as np
import pytest

from conftest import rel_l2, stable_seed
from memcheck import Arena, GUARD_BYTES, MS_ERR_INVALID_ARG, MS_ERR_UNSUPPORTED, MS_ERR_WORKSPACE, MS_OK
from test_gpu_ops import FWD_TOL, GRAD_TOL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
TF = torch.nn.functional

GEN_TOL = 2e-6                       # kernel generation against kernel generation (tests/test_gpu_ops.py)
ATOMIC_ROUTES = ("k_reflect_fold_bwd",)
SLOPE = 0.2


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


def rnd(seed, *shape, scale=1.0):
    r = np.random.default_rng(stable_seed(seed) if isinstance(seed, str) else seed)
    return torch.from_numpy((r.standard_normal(shape) * scale).astype(np.float32))


def arena(nfloats, nbuf=24):
    """An arena for buffers of `nfloats` floats in all."""
    return Arena("cuda", 4 * int(nfloats) + nbuf * (2 * GUARD_BYTES + 1024) + (1 << 20))


def ptr(b):
    return None if b is None else b.ptr


def cpu(t):
    return t.detach().cpu()


def close(got, want, rtol=1e-5, atol=1e-8):
    """np.allclose at the golden loss-gradient test's tolerance (tests/test_gpu_ops.py: test_scalar_losses_golden)."""
    got, want = cpu(got).double().numpy(), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.allclose(got, want, rtol=rtol, atol=atol), float(np.abs(got - want).max())


# ================================================================ (e) stream and reduction kernels

def _pool_ref(kind, x64, k):
    if kind == "422":
        return TF.avg_pool1d(x64, 4, 2, 2, count_include_pad=True)
    if kind == "421":
        return TF.avg_pool1d(x64, 4, 2, 1, count_include_pad=False)
    return TF.avg_pool1d(x64, k)


def pool_case(kind, rows, Lin, add, k=3):
    L, lib = _L()
    s = L.stream()
    name = {"422": "ms_avg_pool1d_4_2_2", "421": "ms_avg_pool1d_4_2_1", "k": "ms_avg_pool1d_k"}[kind]
    fwd, bwd = getattr(lib, name + "_fwd"), getattr(lib, name + "_bwd")
    refused = (kind == "421" and Lin < 2) or (kind == "k" and Lin < k)
    Lout = 1 if refused else {"422": Lin // 2 + 1, "421": (Lin - 2) // 2 + 1, "k": Lin // k}[kind]
    x = rnd("pool%s%d%d" % (kind, rows, Lin), rows, Lin)
    gy = rnd("poolg%s%d%d" % (kind, rows, Lin), rows, Lout)
    ga = rnd("poola%s%d%d" % (kind, rows, Lin), rows, Lin)
    a = arena(rows * (Lin + Lout))
    xb, yb = a.put(x, name="x"), a.take((rows, Lout), "output", name="y")
    tail = (k, s) if kind == "k" else (s,)
    rc, out = a.run_twice(lambda: fwd(xb.ptr, yb.ptr, rows, Lin, *tail), sync)
    a2 = arena(rows * (2 * Lin + Lout))
    gyb, gab = a2.put(gy, name="gy"), (a2.put(ga, name="gx_add") if add and kind != "k" else None)
    gxb = a2.take((rows, Lin), "output", name="gx")
    mid = () if kind == "k" else (ptr(gab),)
    rc2, out2 = a2.run_twice(lambda: bwd(gyb.ptr, *mid, gxb.ptr, rows, Lin, *tail), sync)
    if refused:
        assert rc == MS_ERR_INVALID_ARG and rc2 == MS_ERR_INVALID_ARG
        return
    assert rc == MS_OK and rc2 == MS_OK
    x64 = x.double().view(1, rows, Lin).requires_grad_(True)
    y64 = _pool_ref(kind, x64, k)
    assert tuple(y64.shape) == (1, rows, Lout)
    assert rel_l2(cpu(out["y"]), y64.detach().numpy()[0]) < 1e-6           # (test_avg_pool_golden's gate)
    y64.backward(gy.double().view(1, rows, Lout))
    want = x64.grad[0] + (ga.double() if gab is not None else 0)
    assert rel_l2(cpu(out2["gx"]), want.numpy()) < 1e-6


for _kind in ("422", "421", "k"):
    _syms = {"422": "ms_avg_pool1d_4_2_2", "421": "ms_avg_pool1d_4_2_1", "k": "ms_avg_pool1d_k"}[_kind]
    for _Lin in (1, 2, 3, 4, 5, 1001):
        for _add in ((False, True) if _kind != "k" and _Lin in (4, 1001) else (False,)):
            case("pool%s_L%d%s" % (_kind, _Lin, "_add" if _add else ""), (_syms + "_fwd", _syms + "_bwd"),
                 pool_case, _kind, 7, _Lin, _add)
    # rows * L above 2048 * 256 * 4 elements: the grid-stride loop wraps
    case("pool%s_wrap" % _kind, (_syms + "_fwd", _syms + "_bwd"), pool_case, _kind, 2100, 2003, True)
case("poolk_k7_L30", ("ms_avg_pool1d_k_fwd", "ms_avg_pool1d_k_bwd"), pool_case, "k", 5, 30, False, 7)


def act_bwd_case(act, n, off):
    L, lib = _L()
    ya, gy = rnd("ab%d%d" % (act, n), n), rnd("abg%d%d" % (act, n), n)
    if act == 2:
        ya = torch.tanh(ya)
    a = arena(3 * n)
    yb, gb, ob = a.put(ya, name="y_act", offset_bytes=off), a.put(gy, name="gy"), a.take((n,), "output", name="gpre", offset_bytes=off)
    rc, out = a.run_twice(lambda: lib.ms_act_bwd(yb.ptr, gb.ptr, ob.ptr, n, act, SLOPE, L.stream()), sync)
    assert rc == MS_OK
    y64, g64 = ya.double(), gy.double()
    want = g64 if act == 0 else (torch.where(y64 > 0, g64, SLOPE * g64) if act == 1 else g64 * (1 - y64 * y64))
    assert rel_l2(cpu(out["gpre"]), want.numpy()) < GRAD_TOL


for _act in (0, 1, 2):
    case("act_bwd_act%d" % _act, "ms_act_bwd", act_bwd_case, _act, 4099, 0)
case("act_bwd_lrelu_unaligned_wrap", "ms_act_bwd", act_bwd_case, 1, 2048 * 256 * 4 + 7, 4)


def add_case(n, act, offs):
    """ms_add (act < 0) / ms_add_act: aligned 16-byte path, its 1 .. 3 element tail, operands at 4-byte addresses."""
    L, lib = _L()
    x, y = rnd("add%d" % n, n), rnd("addb%d" % n, n)
    a = arena(3 * n)
    xb, yb = a.put(x, name="a", offset_bytes=offs[0]), a.put(y, name="b", offset_bytes=offs[1])
    ob = a.take((n,), "output", name="out", offset_bytes=offs[2])
    if act < 0:
        rc, out = a.run_twice(lambda: lib.ms_add(xb.ptr, yb.ptr, ob.ptr, n, L.stream()), sync)
        assert rc == MS_OK and np.array_equal(cpu(out["out"]).numpy(), x.numpy() + y.numpy())
        return
    rc, out = a.run_twice(lambda: lib.ms_add_act(xb.ptr, yb.ptr, ob.ptr, n, act, SLOPE, L.stream()), sync)
    assert rc == MS_OK
    z = x.double() + y.double()
    want = z if act == 0 else (TF.leaky_relu(z, SLOPE) if act == 1 else torch.tanh(z))
    assert rel_l2(cpu(out["out"]), want.numpy()) < FWD_TOL


for _n in (1, 3, 4096, 4097, 4099, 2048 * 256 * 4 + 5):
    case("add_n%d" % _n, "ms_add", add_case, _n, -1, (0, 0, 0))
    for _act in ((1,) if _n != 4099 else (0, 1, 2)):
        case("add_act%d_n%d" % (_act, _n), "ms_add_act", add_case, _n, _act, (0, 0, 0))
for _i, _offs in enumerate(((4, 0, 0), (0, 8, 0), (0, 0, 12), (4, 4, 4))):
    case("add_act_unaligned%d" % _i, "ms_add_act", add_case, 4099, 1, _offs)
case("add_unaligned", "ms_add", add_case, 4099, -1, (4, 8, 12))

REDUCE_N = (1, 255, 256 * 8 + 1, 2048 * 256 * 8 + 5)


def reduce_case(kind, n):
    """The five mean reductions with exactly ms_reduce_workspace_bytes(n) of poisoned scratch, and their backward entries."""
    L, lib = _L()
    s = L.stream()
    r, f = rnd("red_r%s%d" % (kind, n), n, scale=0.7), rnd("red_f%s%d" % (kind, n), n, scale=0.7)
    gout, scale = torch.tensor([0.37], dtype=torch.float32), 2.5
    nws = lib.ms_reduce_workspace_bytes(n)
    assert nws > 0
    a = arena(2 * n + nws // 4 + 8)
    rb, fb = a.put(r, name="r"), a.put(f, name="f")
    ob, ws = a.take((1,), "output", name="out"), a.take(nws, "workspace", name="ws")
    fwd = {"hinge_d": lambda: lib.ms_hinge_d_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws, s),
           "neg_mean": lambda: lib.ms_neg_mean_fwd(fb.ptr, n, ob.ptr, ws.ptr, nws, s),
           "l1": lambda: lib.ms_l1_mean_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws, s),
           "ls_g": lambda: lib.ms_ls_g_fwd(fb.ptr, n, ob.ptr, ws.ptr, nws, s),
           "ls_d": lambda: lib.ms_ls_d_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws, s)}[kind]
    rc, out = a.run_twice(fwd, sync)
    assert rc == MS_OK
    r64, f64 = r.double().requires_grad_(True), f.double().requires_grad_(True)
    v64 = {"hinge_d": lambda: (TF.relu(1 - r64) + TF.relu(1 + f64)).mean(), "neg_mean": lambda: (-f64).mean(),
           "l1": lambda: (r64 - f64).abs().mean(), "ls_g": lambda: (0.5 * (f64 - 1) ** 2).mean(),
           "ls_d": lambda: (0.5 * ((r64 - 1) ** 2 + f64 ** 2)).mean()}[kind]()
    assert abs(float(out["out"][0]) - float(v64)) < 1e-6                      # (test_scalar_losses_golden's gate)
    # one byte short of the query: refused, nothing written
    rc, _ = a.run_twice({"hinge_d": lambda: lib.ms_hinge_d_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws - 1, s),
                         "neg_mean": lambda: lib.ms_neg_mean_fwd(fb.ptr, n, ob.ptr, ws.ptr, nws - 1, s),
                         "l1": lambda: lib.ms_l1_mean_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws - 1, s),
                         "ls_g": lambda: lib.ms_ls_g_fwd(fb.ptr, n, ob.ptr, ws.ptr, nws - 1, s),
                         "ls_d": lambda: lib.ms_ls_d_fwd(rb.ptr, fb.ptr, n, ob.ptr, ws.ptr, nws - 1, s)}[kind], sync)
    assert rc == MS_ERR_WORKSPACE
    # backward
    (v64 * float(gout[0]) * scale).backward()
    a2 = arena(4 * n + 8)
    rb, fb, gb = a2.put(r, name="r", offset_bytes=4), a2.put(f, name="f"), a2.put(gout, name="gout")
    if kind == "l1":
        acc0 = rnd("red_acc%d" % n, n)
        gf, gacc = a2.take((n,), "output", name="gf", offset_bytes=8), a2.put(acc0, "accumulate", name="gf_acc")
        rc, out = a2.run_twice(lambda: lib.ms_l1_mean_bwd(rb.ptr, fb.ptr, n, gb.ptr, scale, gf.ptr, 0, s) or
                               lib.ms_l1_mean_bwd(rb.ptr, fb.ptr, n, gb.ptr, scale, gacc.ptr, 1, s), sync)
        assert rc == MS_OK
        close(out["gf"], f64.grad.numpy())
        close(out["gf_acc"], acc0.double().numpy() + f64.grad.numpy())
        return
    gr = a2.take((n,), "output", name="gr") if kind in ("hinge_d", "ls_d") else None
    gf = a2.take((n,), "output", name="gf", offset_bytes=8)
    bwd = {"hinge_d": lambda: lib.ms_hinge_d_bwd(rb.ptr, fb.ptr, n, gb.ptr, scale, ptr(gr), gf.ptr, s),
           "neg_mean": lambda: lib.ms_neg_mean_bwd(n, gb.ptr, scale, gf.ptr, s),
           "ls_g": lambda: lib.ms_ls_g_bwd(fb.ptr, n, gb.ptr, scale, gf.ptr, s),
           "ls_d": lambda: lib.ms_ls_d_bwd(rb.ptr, fb.ptr, n, gb.ptr, scale, ptr(gr), gf.ptr, s)}[kind]
    rc, out = a2.run_twice(bwd, sync)
    assert rc == MS_OK
    close(out["gf"], f64.grad.numpy())
    if gr is not None:
        close(out["gr"], r64.grad.numpy())


_RED_SYMS = {"hinge_d": ("ms_hinge_d_fwd", "ms_hinge_d_bwd"), "neg_mean": ("ms_neg_mean_fwd", "ms_neg_mean_bwd"),
             "l1": ("ms_l1_mean_fwd", "ms_l1_mean_bwd"), "ls_g": ("ms_ls_g_fwd", "ms_ls_g_bwd"),
             "ls_d": ("ms_ls_d_fwd", "ms_ls_d_bwd")}
for _kind, _syms in _RED_SYMS.items():
    for _n in REDUCE_N:
        case("reduce_%s_n%d" % (_kind, _n), _syms, reduce_case, _kind, _n)


def _l1_multi_sizes(vec):
    """MS_L1_MULTI_MAX maps: smaller than a block, exactly one block (2048 backward / 8192 one-pass / 16384 forward
    elements), many blocks plus a tail."""
    base = [4, 100, 2048, 8192, 16384, 3 * 16384 + 20, 2044, 2052, 8188, 16388, 5 * 8192 + 4, 36]
    sizes = (base + [n + 8 for n in base])[:24]
    return sizes if vec else [n + (i % 3) for i, n in enumerate(sizes)]


def l1_multi_case(mode):
    """mode: 'two' = ms_l1_mean_multi_fwd + _bwd, 'one' = ms_l1_mean_multi_fwd_bwd, 'one_unaligned': one map at a 4-byte
    address -> workspace query 0 and MS_ERR_UNSUPPORTED, nothing written."""
    L, lib = _L()
    s = L.stream()
    sizes = _l1_multi_sizes(mode != "two")
    cnt = len(sizes)
    assert cnt == L.L1_MULTI_MAX
    null_gf = cnt // 2
    w = [0.25 + 0.1 * i for i in range(cnt)]
    a = arena(3 * sum(sizes) + 4096, nbuf=3 * cnt + 8)
    d = L.L1MultiDesc()
    d.count = cnt
    rs, fs, gfs = [], [], []
    for i, n in enumerate(sizes):
        r, f = rnd("l1m_r%d" % i, n), rnd("l1m_f%d" % i, n)
        f[::5] = r[::5]                                            # ties: gradient 0
        rs.append(r); fs.append(f)
        off = 4 if (mode == "two" and i % 2) or (mode == "one_unaligned" and i == 3) else 0
        rb, fb = a.put(r, name="r%d" % i, offset_bytes=off), a.put(f, name="f%d" % i)
        gb = None if i == null_gf else a.take((n,), "output", name="gf%d" % i)
        gfs.append(gb)
        d.r[i], d.f[i], d.gf[i], d.n[i], d.w[i] = rb.ptr, fb.ptr, ptr(gb), n, w[i]
    ob = a.take((1,), "output", name="out")
    want = sum(w[i] * float((fs[i].double() - rs[i].double()).abs().mean()) for i in range(cnt))
    gc = 0.37 * 2.5
    if mode == "two":
        nws = lib.ms_l1_mean_multi_workspace_bytes(d)
        ws, gout = a.take(nws, "workspace", name="ws"), a.put(torch.tensor([0.37]), name="gout")
        rc, out = a.run_twice(lambda: lib.ms_l1_mean_multi_fwd(d, ob.ptr, ws.ptr, nws, s) or
                              lib.ms_l1_mean_multi_bwd(d, gout.ptr, 2.5, s), sync)
    else:
        nws = lib.ms_l1_mean_multi_fwd_bwd_workspace_bytes(d)
        if mode == "one_unaligned":
            assert nws == 0
            ws = a.take(4096, "workspace", name="ws")
            rc, _ = a.run_twice(lambda: lib.ms_l1_mean_multi_fwd_bwd(d, ob.ptr, gc, ws.ptr, 4096, s), sync)
            assert rc == MS_ERR_UNSUPPORTED
            return
        ws = a.take(nws, "workspace", name="ws")
        rc, out = a.run_twice(lambda: lib.ms_l1_mean_multi_fwd_bwd(d, ob.ptr, gc, ws.ptr, nws, s), sync)
    assert rc == MS_OK and nws > 0
    assert abs(float(out["out"][0]) - want) <= 1e-5 * abs(want)               # (test_composite_losses_golden's gates)
    for i, n in enumerate(sizes):
        if gfs[i] is not None:
            g = torch.sign(fs[i].double() - rs[i].double()) * (gc * w[i] / n)
            close(out["gf%d" % i], g.numpy(), rtol=1e-5, atol=1e-9)


case("l1_multi_two_calls", ("ms_l1_mean_multi_fwd", "ms_l1_mean_multi_bwd"), l1_multi_case, "two")
case("l1_multi_one_pass", "ms_l1_mean_multi_fwd_bwd", l1_multi_case, "one")
case("l1_multi_one_pass_unaligned_map", "ms_l1_mean_multi_fwd_bwd", l1_multi_case, "one_unaligned")


def judge_multi_case(kind):
    L, lib = _L()
    s = L.stream()
    ns = [32, 17, 9, 1, 300, 255, 257, 5000]
    a = arena(4 * sum(ns) + 16, nbuf=40)
    d = L.JudgeMultiDesc()
    d.count, d.kind = len(ns), kind
    rs, fs, want = [], [], 0.0
    for i, n in enumerate(ns):
        r, f = rnd("jm_r%d" % i, n, scale=2.0), rnd("jm_f%d" % i, n, scale=2.0)
        rs.append(r); fs.append(f)
        off = 4 * (i % 4)
        d.f[i], d.n[i] = a.put(f, name="f%d" % i, offset_bytes=off).ptr, n
        d.gf[i] = a.take((n,), "output", name="gf%d" % i).ptr if i != 2 else None
        if kind == L.JUDGE_HINGE_D:
            d.r[i] = a.put(r, name="r%d" % i).ptr
            d.gr[i] = a.take((n,), "output", name="gr%d" % i, offset_bytes=off).ptr if i != 5 else None
            want += float((TF.relu(1 - r.double()) + TF.relu(1 + f.double())).mean())
        else:
            want += float((-f.double()).mean())
    ob, gout = a.take((1,), "output", name="out"), a.put(torch.tensor([0.7]), name="gout")
    rc, out = a.run_twice(lambda: lib.ms_judge_loss_multi_fwd(d, ob.ptr, s) or lib.ms_judge_loss_multi_bwd(d, gout.ptr, 1.5, s), sync)
    assert rc == MS_OK
    assert abs(float(out["out"][0]) - want) <= 1e-6 * max(1.0, abs(want))     # (test_judge_loss_multi_matches_single_terms)
    for i, n in enumerate(ns):
        g = 0.7 * 1.5 / n
        if "gf%d" % i in out:
            close(out["gf%d" % i], (torch.where(1 + fs[i].double() > 0, g, 0.0) if kind == L.JUDGE_HINGE_D
                                    else torch.full((n,), -g, dtype=torch.float64)).numpy())
        if "gr%d" % i in out:
            close(out["gr%d" % i], torch.where(1 - rs[i].double() > 0, -g, 0.0).numpy())


case("judge_multi_hinge_d", ("ms_judge_loss_multi_fwd", "ms_judge_loss_multi_bwd"), judge_multi_case, 0)
case("judge_multi_neg_mean", ("ms_judge_loss_multi_fwd", "ms_judge_loss_multi_bwd"), judge_multi_case, 1)


def weighted_sum_case(n, off):
    L, lib = _L()
    t, c = rnd("ws_t%d" % n, n), rnd("ws_c%d" % n, n)
    a = arena(2 * n + 8)
    tb, cb, ob = a.put(t, name="terms", offset_bytes=off), a.put(c, name="coef"), a.take((1,), "output", name="out", offset_bytes=off)
    rc, out = a.run_twice(lambda: lib.ms_weighted_sum(tb.ptr, cb.ptr, n, ob.ptr, L.stream()), sync)
    want = float((t.double() * c.double()).sum())
    assert rc == MS_OK and abs(float(out["out"][0]) - want) <= 1e-5 * abs(want)  # (test_composite_losses_golden's gate)


case("weighted_sum_n1", "ms_weighted_sum", weighted_sum_case, 1, 0)
case("weighted_sum_n5_unaligned", "ms_weighted_sum", weighted_sum_case, 5, 4)


def adam_case(n, off):
    """n % 4 in {0, 1, 3}, grad_scale != 1; a bucket at a 4-byte address is refused (include/msynth.h: one flat bucket from
    the allocator) and nothing is written."""
    L, lib = _L()
    p, g, m = rnd("ad_p%d" % n, n), rnd("ad_g%d" % n, n), rnd("ad_m%d" % n, n, scale=0.1)
    v = rnd("ad_v%d" % n, n, scale=0.1).abs()
    a = arena(4 * n + 8)
    pb, gb = a.put(p, "accumulate", name="p", offset_bytes=off), a.put(g, name="g")
    mb, vb = a.put(m, "accumulate", name="m"), a.put(v, "accumulate", name="v")
    sb = a.put(torch.tensor([4], dtype=torch.int32), "accumulate", name="step")
    lr, b1, b2, eps, gs = 1e-3, 0.5, 0.9, 1e-8, 0.25
    rc, out = a.run_twice(lambda: lib.ms_adam_step(pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, lr, b1, b2, eps, gs, sb.ptr, L.stream()), sync)
    if off:
        assert rc == MS_ERR_INVALID_ARG
        return
    assert rc == MS_OK and int(out["step"][0]) == 5
    g64 = g.double() * gs
    m64, v64 = b1 * m.double() + (1 - b1) * g64, b2 * v.double() + (1 - b2) * g64 * g64
    p64 = p.double() - (lr / (1 - b1 ** 5)) * m64 / (v64.sqrt() / np.sqrt(1 - b2 ** 5) + eps)
    for nm, w64 in (("p", p64), ("m", m64), ("v", v64)):
        assert rel_l2(cpu(out[nm]), w64.numpy()) < 1e-6, nm                   # (test_adam_golden's gate)


for _n in (4096, 4097, 4099, 3):
    case("adam_n%d" % _n, "ms_adam_step", adam_case, _n, 0)
case("adam_unaligned_refused", "ms_adam_step", adam_case, 4099, 4)


def _wn_ref(v, g, gw):
    v64, g64 = v.double().requires_grad_(True), g.double().requires_grad_(True)
    w64 = g64[:, None] * v64 / v64.norm(dim=1, keepdim=True)
    w64.backward(gw.double())
    return w64.detach(), v64.grad, g64.grad


def weight_norm_case(multi, beta):
    L, lib = _L()
    s = L.stream()
    shapes = [(7, 300), (3, 2), (1, 1025), (64, 20), (5, 256)] if multi else [(7, 300)]
    a = arena(6 * sum(r * c for r, c in shapes) + 64, nbuf=8 * len(shapes))
    d, d2 = L.WnMultiDesc(), L.WnMultiDesc()
    d.count = d2.count = len(shapes)
    refs, bufs = [], []
    for i, (r, c) in enumerate(shapes):
        v, g, gw = rnd("wn_v%d" % i, r, c), rnd("wn_g%d" % i, r), rnd("wn_gw%d" % i, r, c)
        gv0, gg0 = rnd("wn_gv%d" % i, r, c), rnd("wn_gg%d" % i, r)
        off = 4 * (i % 3)
        vb, gb = a.put(v, name="v%d" % i, offset_bytes=off), a.put(g, name="g%d" % i)
        wb, gwb = a.take((r, c), "output", name="w%d" % i, offset_bytes=off), a.put(gw, name="gw%d" % i, offset_bytes=4)
        gvb = a.put(gv0, "accumulate", name="gv%d" % i) if beta else a.take((r, c), "output", name="gv%d" % i)
        ggb = a.put(gg0, "accumulate", name="gg%d" % i) if beta else a.take((r,), "output", name="gg%d" % i)
        bufs.append((vb, gb, wb, gwb, gvb, ggb))
        refs.append(_wn_ref(v, g, gw) + (gv0.double() * beta, gg0.double() * beta))
        for dd, ob in ((d, wb), (d2, gwb)):
            dd.v[i], dd.g[i], dd.out[i], dd.gv[i], dd.gg[i], dd.rows[i], dd.cols[i] = vb.ptr, gb.ptr, ob.ptr, gvb.ptr, ggb.ptr, r, c
    if multi:
        call = lambda: lib.ms_weight_norm_multi_fwd(d, s) or lib.ms_weight_norm_multi_bwd(d2, float(beta), s)
    else:
        vb, gb, wb, gwb, gvb, ggb = bufs[0]
        r, c = shapes[0]
        call = lambda: (lib.ms_weight_norm_fwd(vb.ptr, gb.ptr, wb.ptr, r, c, s) or
                        lib.ms_weight_norm_bwd(vb.ptr, gb.ptr, gwb.ptr, gvb.ptr, ggb.ptr, r, c, float(beta), s))
    rc, out = a.run_twice(call, sync)
    assert rc == MS_OK
    for i, (w64, gv64, gg64, gv0, gg0) in enumerate(refs):
        assert rel_l2(cpu(out["w%d" % i]), w64.numpy()) < FWD_TOL
        assert rel_l2(cpu(out["gv%d" % i]), (gv64 + gv0).numpy()) < GRAD_TOL
        assert rel_l2(cpu(out["gg%d" % i]), (gg64 + gg0).numpy()) < GRAD_TOL


for _beta in (0, 1):
    case("weight_norm_beta%d" % _beta, ("ms_weight_norm_fwd", "ms_weight_norm_bwd"), weight_norm_case, False, _beta)
    case("weight_norm_multi_beta%d" % _beta, ("ms_weight_norm_multi_fwd", "ms_weight_norm_multi_bwd"), weight_norm_case, True, _beta)


LINE_PHASES = {"s2": [[0, -1], [1, 0]], "s1": [[1, 0, -1]]}


def lines_case(geom, shape, off):
    """ms_lines_stack / _fold / _interleave; a buffer at a 4-byte address is refused (16-byte aligned by the header)."""
    from featuresynth._ops import prims as P
    from test_gpu_lines import _ref_stack
    L, lib = _L()
    s = L.stream()
    phases = LINE_PHASES[geom]
    B, H, C, W = shape
    x = rnd("lines%s%s" % (geom, shape), *shape)
    d = P.lines_desc(shape, phases)
    nph, taps = len(phases), len(phases[0])
    g = rnd("linesg%s%s" % (geom, shape), nph, B * H, taps * C, W)
    a = arena(2 * x.numel() + 4 * g.numel())
    xb, ob = a.put(x, name="x", offset_bytes=off), a.take(tuple(g.shape), "output", name="stack")
    gb, gxb = a.put(g, name="gstack"), a.take(shape, "output", name="gx", offset_bytes=off)
    n = taps * C * W
    ib = a.take((B * H, nph, n), "output", name="interleaved")
    bb = a.take((nph, B * H, n), "output", name="back", offset_bytes=off)
    calls = [lambda: lib.ms_lines_stack(d, xb.ptr, ob.ptr, s), lambda: lib.ms_lines_fold(d, gb.ptr, gxb.ptr, s),
             lambda: lib.ms_lines_interleave(gb.ptr, ib.ptr, B * H, nph, n, 0, s)]
    if off:
        for c in (calls[0], calls[1], lambda: lib.ms_lines_interleave(gb.ptr, bb.ptr, B * H, nph, n, 1, s)):
            rc, _ = a.run_twice(c, sync)
            assert rc == MS_ERR_INVALID_ARG
        return
    rc, out = a.run_twice(lambda: calls[0]() or calls[1]() or calls[2]() or
                          lib.ms_lines_interleave(ib.ptr, bb.ptr, B * H, nph, n, 1, s), sync)
    assert rc == MS_OK
    xr = x.clone().requires_grad_(True)
    ref = _ref_stack(xr, phases)
    assert torch.equal(cpu(out["stack"]), ref.detach())
    ref.backward(g)
    assert rel_l2(cpu(out["gx"]), xr.grad.numpy()) < 1e-6                    # (tests/test_gpu_lines.py's gate)
    assert torch.equal(cpu(out["interleaved"]), g.reshape(nph, B * H, n).permute(1, 0, 2).contiguous())
    assert torch.equal(cpu(out["back"]), g.reshape(nph, B * H, n))


_LINE_SYMS = ("ms_lines_stack", "ms_lines_fold", "ms_lines_interleave")
for _geom in ("s2", "s1"):
    case("lines_%s_ragged" % _geom, _LINE_SYMS, lines_case, _geom, (2, 5, 24, 8), 0)
    case("lines_%s_one_row" % _geom, _LINE_SYMS, lines_case, _geom, (3, 1, 8, 12), 0)
case("lines_unaligned_refused", _LINE_SYMS, lines_case, "s2", (2, 5, 24, 8), 4)


def audio2mel_case(B, N, n_mel, off):
    from featuresynth.feature.feature import slaney_mel_basis
    from test_gpu_audio2mel_grad import a2m64, noise_with_silence
    L, lib = _L()
    s = L.stream()
    n_fft, hop = 1024, 256
    frames = lib.ms_audio2mel_frames(N, n_fft, hop)
    assert frames > 0
    x = torch.from_numpy(noise_with_silence(B, N, seed=N + n_mel))
    nn_ = torch.arange(n_fft, dtype=torch.float64)
    window = (0.5 - 0.5 * torch.cos(2.0 * np.pi * nn_ / n_fft)).float()
    basis = torch.from_numpy(slaney_mel_basis(22050, n_fft, n_mel))
    G = rnd("a2m_g%d" % N, B, n_mel, frames)
    nws = lib.ms_audio2mel_bwd_workspace_bytes(B, N, n_fft, hop)
    assert nws > 0
    a = arena(3 * B * N + 2 * B * n_mel * frames + n_fft + basis.numel() + nws // 4)
    xb, wb, bb = a.put(x.view(B, N), name="audio", offset_bytes=off), a.put(window, name="window"), a.put(basis, name="mel_basis", offset_bytes=off)
    ob, gb = a.take((B, n_mel, frames), "output", name="out", offset_bytes=off), a.put(G, name="grad_out")
    gab, ws = a.take((B, N), "output", name="grad_audio", offset_bytes=off), a.take(nws, "workspace", name="ws")
    rc, out = a.run_twice(lambda: lib.ms_audio2mel_fwd(xb.ptr, B, N, wb.ptr, n_fft, hop, bb.ptr, n_mel, ob.ptr, s) or
                          lib.ms_audio2mel_bwd(xb.ptr, B, N, wb.ptr, n_fft, hop, bb.ptr, n_mel, gb.ptr, gab.ptr, ws.ptr, nws, s), sync)
    assert rc == MS_OK
    x64 = x.double().requires_grad_(True)
    y64 = a2m64(x64, window.double(), basis.double(), n_fft, hop)
    (y64 * G.double()).sum().backward()
    assert np.abs(cpu(out["out"]).numpy() - y64.detach().numpy()).max() < 2e-4          # (test_audio2mel_golden's gate)
    errs = [rel_l2(cpu(out["grad_audio"][b]), x64.grad[b, 0].numpy()) for b in range(B)]
    assert max(errs) <= 1e-4, errs                                                       # (tests/test_gpu_audio2mel_grad.py's gate)
    rc, _ = a.run_twice(lambda: lib.ms_audio2mel_bwd(xb.ptr, B, N, wb.ptr, n_fft, hop, bb.ptr, n_mel, gb.ptr, gab.ptr, ws.ptr,
                                                     nws - 1, s), sync)
    assert rc == MS_ERR_WORKSPACE


_A2M = ("ms_audio2mel_fwd", "ms_audio2mel_bwd")
case("audio2mel_b2_n4096", _A2M, audio2mel_case, 2, 4096, 80, 0)
case("audio2mel_b3_odd_n128", _A2M, audio2mel_case, 3, 2049, 128, 0)


def stft_case(B, N, res):
    from test_gpu_stft_loss import MIN_POWER, pair_loss_float64, real_rows, fake_rows, stft_mag_ref
    L, lib = _L()
    s = L.stream()
    n_fft, hop, win = res
    frames, bins = lib.ms_stft_frames(N, n_fft, hop), n_fft // 2 + 1
    assert frames == 1 + N // hop
    x = torch.from_numpy(real_rows(B, N, seed=N + hop))
    window = torch.zeros(n_fft)
    left = (n_fft - win) // 2
    window[left:left + win] = (0.5 - 0.5 * torch.cos(2.0 * np.pi * torch.arange(win, dtype=torch.float64) / win)).float()
    G = rnd("stft_g%d%d" % (N, n_fft), B, frames, bins)
    nws = lib.ms_stft_mag_bwd_workspace_bytes(B, N, n_fft, hop)
    assert nws == 4 * B * frames * n_fft
    a = arena(2 * B * N + 2 * B * frames * bins + n_fft + nws // 4)
    xb, wb = a.put(x.view(B, N), name="audio"), a.put(window, name="window")
    mb, gb = a.take((B, frames, bins), "output", name="mag"), a.put(G, name="grad_mag")
    gab, ws = a.take((B, N), "output", name="grad_audio"), a.take(nws, "workspace", name="ws")
    rc, out = a.run_twice(lambda: lib.ms_stft_mag_fwd(xb.ptr, B, N, wb.ptr, n_fft, hop, MIN_POWER, mb.ptr, s) or
                          lib.ms_stft_mag_bwd(xb.ptr, B, N, wb.ptr, n_fft, hop, MIN_POWER, gb.ptr, gab.ptr, ws.ptr, nws, s), sync)
    assert rc == MS_OK
    x64 = x.double().requires_grad_(True)
    y64 = stft_mag_ref(x64, n_fft, hop, win)                                  # (B, bins, frames)
    (y64 * G.double().transpose(1, 2)).sum().backward()
    fwd = [rel_l2(cpu(out["mag"][b]).t(), y64[b].detach().numpy()) for b in range(B)]
    bwd = [rel_l2(cpu(out["grad_audio"][b]), x64.grad[b, 0].numpy()) for b in range(B)]
    assert max(fwd) <= 1e-4 and max(bwd) <= 1e-4, (fwd, bwd)                    # (tests/test_gpu_stft_loss.py's gates)
    rc, _ = a.run_twice(lambda: lib.ms_stft_mag_bwd(xb.ptr, B, N, wb.ptr, n_fft, hop, MIN_POWER, gb.ptr, gab.ptr, ws.ptr,
                                                    nws - 4, s), sync)
    assert rc == MS_ERR_WORKSPACE
    # the pair loss on these magnitudes against magnitudes of other audio
    Fm = out["mag"].cpu()
    Rm = stft_mag_ref(torch.from_numpy(fake_rows(B, N, seed=5)), n_fft, hop, win).transpose(1, 2).contiguous().float()
    n = Fm.numel()
    nws = lib.ms_stft_pair_loss_workspace_bytes(n)
    a2 = arena(3 * n + nws // 4 + 64)
    fb, rb = a2.put(Fm, name="f", offset_bytes=4), a2.put(Rm, name="r")
    rss, sums, ob = a2.take((1,), "output", name="r_sumsq"), a2.take((3,), "output", name="sums"), a2.take((1,), "output", name="out")
    gout, gf = a2.put(torch.tensor([0.6]), name="gout"), a2.take((n,), "output", name="grad_f", offset_bytes=8)
    ws = a2.take(nws, "workspace", name="ws")
    rc, out = a2.run_twice(lambda: lib.ms_stft_pair_loss_target(rb.ptr, n, rss.ptr, ws.ptr, nws, s) or
                           lib.ms_stft_pair_loss_fwd(fb.ptr, rb.ptr, n, rss.ptr, 0.25, 3.0, sums.ptr, ob.ptr, ws.ptr, nws, s) or
                           lib.ms_stft_pair_loss_bwd(fb.ptr, rb.ptr, n, sums.ptr, gout.ptr, 0.25, 3.0, gf.ptr, s), sync)
    assert rc == MS_OK
    sc64, lm64, dF64 = pair_loss_float64(Fm.numpy(), Rm.numpy(), 0.25, 3.0)
    want = 0.25 * sc64 + 3.0 * lm64
    r2 = float((Rm.double() ** 2).sum())
    assert abs(float(out["r_sumsq"][0]) - r2) <= 1e-5 * r2
    assert abs(float(out["out"][0]) - want) <= 1e-4 * want
    assert rel_l2(cpu(out["grad_f"]), 0.6 * dF64.reshape(-1)) <= 1e-4
    rc, _ = a2.run_twice(lambda: lib.ms_stft_pair_loss_fwd(fb.ptr, rb.ptr, n, rss.ptr, 0.25, 3.0, sums.ptr, ob.ptr, ws.ptr,
                                                           nws - 1, s), sync, )
    assert rc == MS_ERR_WORKSPACE


_STFT = ("ms_stft_mag_fwd", "ms_stft_mag_bwd", "ms_stft_pair_loss_target", "ms_stft_pair_loss_fwd", "ms_stft_pair_loss_bwd")
case("stft_64_16_b2_n1000", _STFT, stft_case, 2, 1000, (64, 16, 64))
case("stft_512_50_b1_n2049", _STFT, stft_case, 1, 2049, (512, 50, 240))


def resample_case(orig, target):
    from featuresynth.feature.feature import KAISER_BEST, sinc_window
    from oracle import oracle as O
    L, lib = _L()
    s = L.stream()
    rows, n = 3, 3000
    t = np.arange(n) / orig
    r = np.random.default_rng(stable_seed("rs%d" % orig))
    x = np.stack([0.4 * np.sin(2 * np.pi * 220 * t) + 0.1 * r.standard_normal(n), 0.05 * r.standard_normal(n),
                  np.zeros(n)]).astype(np.float32)
    ratio = float(target) / float(orig)
    win, num_table = sinc_window(**KAISER_BEST)
    if ratio < 1:
        win = win * ratio
    delta = np.zeros_like(win)
    delta[:-1] = np.diff(win)
    ref = O.resample_kaiser_best(x, orig, target)
    n_out = ref.shape[-1]
    a = arena(rows * (n + 2 * n_out) + 2 * win.size + 16)
    xb = a.put(torch.from_numpy(x), name="x", offset_bytes=4)
    wb = a.put(torch.from_numpy(win.astype(np.float32)), name="interp_win", offset_bytes=8)
    db = a.put(torch.from_numpy(delta.astype(np.float32)), name="interp_delta")
    yb = a.take((rows, n_out), "output", name="y", offset_bytes=4)
    rc, out = a.run_twice(lambda: lib.ms_resample_sinc_fwd(xb.ptr, rows, n, yb.ptr, n_out, ratio, wb.ptr, db.ptr, win.size,
                                                           num_table, s), sync)
    assert rc == MS_OK
    y = cpu(out["y"]).numpy()
    assert np.abs(y - ref).max() < 2e-5 * max(1.0, np.abs(ref).max())                    # (test_audio_frontend_vs_oracle's gates)
    # in place: the role is accumulate; one all-zero row stays zero
    a2 = arena(rows * n_out + 16)
    pb, ws = a2.put(torch.from_numpy(y), "accumulate", name="x", offset_bytes=4), a2.take(4 * rows, "workspace", name="ws")
    rc, out = a2.run_twice(lambda: lib.ms_peak_normalize(pb.ptr, rows, n_out, 0.95, ws.ptr, s), sync)
    assert rc == MS_OK
    peak = np.abs(y).max(axis=1, keepdims=True)
    want = np.where(peak > 0, y.astype(np.float64) * 0.95 / np.maximum(peak, 1e-300), 0.0)
    got = cpu(out["x"]).numpy()
    assert np.abs(got - want).max() < 5e-5 and float(np.abs(got[2]).max()) == 0.0
    assert abs(float(np.abs(got[0]).max()) - 0.95) < 1e-5


case("resample_down_and_normalize", ("ms_resample_sinc_fwd", "ms_peak_normalize"), resample_case, 44100, 22050)
case("resample_up_and_normalize", ("ms_resample_sinc_fwd", "ms_peak_normalize"), resample_case, 11025, 22050)

# ================================================================ (a) (b) convs and transposed convs through the dispatch plan

def _stem(name):
    return name.split("<")[0].strip()


def profiled(fn, notes):
    """fn() inside a profile session of its own; appends (kernel noted last, launches) to notes."""
    L, lib = _L()

    def call():
        rec = L.ProfileRecord()
        lib.ms_profile_take(ctypes.byref(rec))
        lib.ms_profile_kernels(1)
        try:
            rc = fn()
            lib.ms_profile_take(ctypes.byref(rec))
        finally:
            lib.ms_profile_kernels(0)
        notes.append((rec.kernel.decode(), int(rec.kernels)))
        return rc
    return call


def _workspace(a, nws, mode):
    """-> (buffer or None, pointer, size passed): 'exact' = the query's byte count, 'plus4' = the same bytes at a 4-byte
    address, 'null' = no workspace."""
    if mode == "null" or nws == 0:
        return None, None, 0
    b = a.take(nws, "workspace", name="ws", offset_bytes=4 if mode == "plus4" else 0)
    return b, b.ptr, nws


def conv_case(shape, which, stem=None, offs=None, ws_mode="exact", differs=None, min_kernels=0, expect=MS_OK, note_re=None,
              env=None):
    """One conv geometry through ms_conv1d_fwd (which 0: plain, then with residual and y_act), _bwd_data (1: without and with
    gx_add) or _bwd_weight (2: beta 0 and 1).  stem: the kernel the case exists for -- the plain aligned call must note it.
    offs: {operand: byte offset} for the placement cases; then MS_OK with right values or a refusal that wrote nothing, and
    differs = the aligned run's stem that must NOT be noted; note_re: what the note must match (the instantiation the launcher
    records, e.g. its dword form); expect: the status (every plan below ends in a route that takes the call, so MS_OK unless the
    case says otherwise); env: tuning switches set for the case (the library reads them on every call)."""
    import os
    for k, v in (env or {}).items():
        os.environ[k] = v
    try:
        _conv_case(shape, which, stem, offs, ws_mode, differs, min_kernels, expect, note_re)
    finally:
        for k in (env or {}):
            del os.environ[k]


def _conv_case(shape, which, stem, offs, ws_mode, differs, min_kernels, expect, note_re):
    import re
    from oracle import oracle as O
    L, lib = _L()
    s = L.stream()
    offs = offs or {}
    name, B, Cin, Lg, Cout, K, st, pad, dil, g, act, refl = shape
    r = np.random.default_rng(stable_seed(name))
    x = r.standard_normal((B, Cin, Lg)).astype(np.float32)
    w = (r.standard_normal((Cout, Cin // g, K)) * 0.1).astype(np.float32)
    b = (r.standard_normal((Cout,)) * 0.1).astype(np.float32)
    pm = O.PAD_REFLECT if refl else O.PAD_ZERO
    d = L.ConvDesc(B, Cin, Lg, Cout, K, st, pad, dil, g, 1 if refl else 0, act, SLOPE, 0)
    Lo = lib.ms_conv1d_out_len(d)
    ya = O.conv1d_fwd(x, w, b, st, pad, dil, g, pm, act).astype(np.float32)
    assert ya.shape == (B, Cout, Lo)
    res = r.standard_normal(ya.shape).astype(np.float32)
    gy = r.standard_normal(ya.shape).astype(np.float32)
    add = r.standard_normal(x.shape).astype(np.float32)
    gw0 = r.standard_normal(w.shape).astype(np.float32)
    gb0 = r.standard_normal(b.shape).astype(np.float32)
    query = lib.ms_conv1d_kernel_name(d, which).decode()
    nws = lib.ms_conv1d_workspace_bytes(d, which)
    floats = 3 * x.size + 4 * ya.size + 3 * w.size + nws // 4 + 64
    o = lambda k: offs.get(k, 0)
    T = torch.from_numpy
    for variant in (0, 1):
        a = arena(floats)
        notes = []
        if which == 0:
            xb, wb, bb = a.put(T(x), name="x", offset_bytes=o("x")), a.put(T(w), name="w", offset_bytes=o("w")), a.put(T(b), name="bias")
            rb = a.put(T(res), name="residual", offset_bytes=o("residual")) if variant else None
            yb = a.take(ya.shape, "output", name="y", offset_bytes=o("y"))
            yab = a.take(ya.shape, "output", name="y_act", offset_bytes=o("y_act")) if variant else None
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_conv1d_fwd(d, xb.ptr, wb.ptr, bb.ptr, ptr(rb), yb.ptr, ptr(yab), wsp, wsn, s)
            tol = None
        elif which == 1:
            gyb, wb = a.put(T(gy), name="gy", offset_bytes=o("gy")), a.put(T(w), name="w", offset_bytes=o("w"))
            yab = a.put(T(ya), name="y_act", offset_bytes=o("y_act")) if act else None
            ab = a.put(T(add), name="gx_add", offset_bytes=o("gx_add")) if variant else None
            gxb = a.take(x.shape, "output", name="gx", offset_bytes=o("gx"))
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_conv1d_bwd_data(d, gyb.ptr, ptr(yab), wb.ptr, ptr(ab), gxb.ptr, wsp, wsn, s)
            # float atomics in the reflection fold: two mirrored taps meet on one sample only when Lin <= 2 pad + 1
            tol = (ATOMIC_ROUTES[0], GRAD_TOL) if refl and Lg <= 2 * pad + 1 else None
        else:
            xb, gyb = a.put(T(x), name="x", offset_bytes=o("x")), a.put(T(gy), name="gy", offset_bytes=o("gy"))
            yab = a.put(T(ya), name="y_act", offset_bytes=o("y_act")) if act else None
            if variant:
                gwb, gbb = a.put(T(gw0), "accumulate", name="gw", offset_bytes=o("gw")), a.put(T(gb0), "accumulate", name="gb", offset_bytes=o("gb"))
            else:
                gwb, gbb = a.take(w.shape, "output", name="gw", offset_bytes=o("gw")), a.take(b.shape, "output", name="gb", offset_bytes=o("gb"))
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_conv1d_bwd_weight(d, xb.ptr, gyb.ptr, ptr(yab), gwb.ptr, gbb.ptr, float(variant), wsp, wsn, s)
            tol = None
        rc, out = a.run_twice(profiled(call, notes), sync, tol)
        plain = not offs and ws_mode == "exact"
        assert rc == expect, "status %d, expected %d (%s)" % (rc, expect, notes)
        if rc != MS_OK:
            continue
        # (the recorded form is looked at in the variant that has the moved operand and stays on the route: a forward with
        #  residual / y_act leaves the grouped routes, gx_add exists only in the second backward-data variant)
        if note_re and variant == (1 if which == 1 and offs and set(offs) == {"gx_add"} else 0):
            assert re.search(note_re, notes[0][0]), (note_re, notes)
        if variant == 0 and plain and stem:
            assert _stem(notes[0][0]) == _stem(query) and _stem(query) == stem, (notes, query, stem)
            assert notes[0][1] >= min_kernels, notes
        if variant == 0 and differs:
            assert _stem(notes[0][0]) != differs, "the declined route's kernel ran: %s" % (notes,)
        if which == 0:
            assert rel_l2(cpu(out["y"]), ya.astype(np.float64) + (res if variant else 0)) < FWD_TOL
            if variant:
                assert rel_l2(cpu(out["y_act"]), ya) < FWD_TOL
        elif which == 1:
            gp = O.act_bwd(ya, gy, act)
            ref = O.conv1d_bwd_data(gp, w, x.shape, st, pad, dil, g, pm)
            assert rel_l2(cpu(out["gx"]), ref.astype(np.float64) + (add if variant else 0)) < GRAD_TOL
        else:
            gp = O.act_bwd(ya, gy, act)
            gw_ref, gb_ref = O.conv1d_bwd_weight(x, gp, w.shape, st, pad, dil, g, pm)
            assert rel_l2(cpu(out["gw"]), gw_ref.astype(np.float64) + (gw0 if variant else 0)) < GRAD_TOL
            assert rel_l2(cpu(out["gb"]), gb_ref.astype(np.float64) + (gb0 if variant else 0)) < GRAD_TOL


_CONV_SYMS = ("ms_conv1d_fwd", "ms_conv1d_bwd_data", "ms_conv1d_bwd_weight")
# name, B, Cin, L, Cout, K, stride, pad, dil, groups, act, reflect (the layout of HOT_CONVS in tests/test_gpu_ops.py, whose
# smallest shape per route is used where it has one)
_S = {
    "judge_l17": ("d_judge_l17", 3, 1024, 17, 1, 3, 1, 1, 1, 1, 0, False),
    "first_b1_l4": ("cs_first_l4", 1, 80, 4, 512, 7, 1, 3, 1, 1, 1, True),
    "k5_l17_pad4": ("d_k5_l17_padded", 61, 256, 17, 272, 5, 1, 2, 1, 1, 1, False),
    "k3_l16_rows": ("r3_k3_l16_r8", 9, 64, 16, 64, 3, 1, 1, 1, 1, 1, False),
    "mfma_m48": ("mfma_m48_k120", 3, 40, 77, 48, 3, 1, 3, 3, 1, 1, False),
    "mfma_m96_k5": ("mfma_m96_k5", 2, 36, 41, 96, 5, 1, 2, 1, 1, 0, False),
    "c32_l64": ("w32_d3_short", 5, 32, 64, 32, 3, 1, 3, 3, 1, 1, False),
    "g4x4_l65": ("g3_og4_l65", 2, 512, 65, 512, 41, 4, 20, 1, 128, 1, False),
    "g4_l260": ("g3_l260_wrap", 3, 16, 260, 64, 41, 4, 20, 1, 4, 1, False),
    "g16_tanh": ("mc_g16_tanh", 2, 64, 64, 256, 41, 4, 20, 1, 16, 2, False),
    "g16_og4_tanh": ("mc_g16_og4_tanh", 2, 64, 64, 64, 41, 4, 20, 1, 16, 2, False),
    "last_k7_odd": ("g_last_k7_tanh_odd", 3, 32, 1301, 1, 7, 1, 3, 1, 1, 2, False),
    "k15_short": ("d_k15_short", 2, 1, 9, 16, 15, 1, 7, 1, 1, 1, False),
    "direct_s2": ("mc_direct_s2", 2, 6, 50, 10, 3, 2, 1, 1, 1, 1, False),
    "reflect_k7": ("mfma_m160_k7_reflect", 2, 24, 50, 160, 7, 1, 3, 1, 1, 2, True),
    "reflect_k3_l5": ("w_reflect_k3_l5", 4, 64, 5, 64, 3, 1, 1, 1, 1, 0, True),
    "wshort_k5": ("w_short_k5_l64_tanh", 8, 36, 64, 96, 5, 1, 2, 1, 1, 2, True),
    "w5_l7": ("w5_l7", 2, 256, 7, 256, 5, 1, 2, 1, 1, 1, False),
    "w5_l12_split": ("w5_l12_noact", 5, 320, 12, 256, 5, 1, 2, 1, 1, 0, False),
    "wrows_l9": ("wrows_k3_l9_d3", 11, 96, 9, 80, 3, 1, 3, 3, 1, 1, False),
    "wrows3_l4096": ("r3_c64_l4096_d3", 1, 64, 4096, 64, 3, 1, 3, 3, 1, 1, False),
}
# (route of api.hip's Kind enum, shape, which, kernel stem)
CONV_ROUTES = [
    ("F_THIN_SHORT", "judge_l17", 0, "k_thin_short_fwd"), ("F_SMALL", "first_b1_l4", 0, "k_conv_small"),
    ("F_PAD4", "k5_l17_pad4", 0, "k_conv_rows3"), ("F_MFMA", "k3_l16_rows", 0, "k_conv_rows3"),
    ("F_MFMA_rows1", "mfma_m48", 0, "k_conv_mfma_rows"), ("F_MFMA_igemm", "mfma_m96_k5", 0, "k_igemm_conv"),
    ("F_MFMA_rows2", "c32_l64", 0, "k_conv_rows2"), ("F_G4", "g4x4_l65", 0, "k_g4_fwd"), ("F_G3", "g4_l260", 0, "k_gconv_split_fwd"),
    ("F_G", "g16_tanh", 0, "k_gconv_mfma_fwd"), ("F_THIN", "last_k7_odd", 0, "k_thin_reduce"), ("F_DIRECT", "k15_short", 0, "k_conv1d_fwd_direct"),
    ("F_DIRECT_s2", "direct_s2", 0, "k_conv1d_fwd_direct"),
    ("D_PAD4", "k5_l17_pad4", 1, "k_conv_rows3"), ("D_MFMA", "k3_l16_rows", 1, "k_conv_rows3"), ("D_G4", "g4x4_l65", 1, "k_g4_bwd_data"),
    ("D_G3", "g4_l260", 1, "k_gconv_split_bwd_data"), ("D_G", "g16_og4_tanh", 1, "k_gconv_mfma_bwd_data"),
    ("D_THIN", "last_k7_odd", 1, "k_thin_expand"), ("D_THIN_k15", "k15_short", 1, "k_thin_reduce"),
    ("D_DIRECT", "judge_l17", 1, "k_conv1d_bwd_data_direct"), ("D_DIRECT_s2", "direct_s2", 1, "k_conv1d_bwd_data_direct"),
    ("D_DIRECT_reflect_fold", "reflect_k7", 1, "k_conv1d_bwd_data_direct"), ("D_MFMA_reflect_fold_l5", "reflect_k3_l5", 1, "k_conv_rows3"),
    ("W_THIN", "last_k7_odd", 2, "k_thin_wgrad"), ("W_THIN_k15", "k15_short", 2, "k_thin_wgrad"), ("W_SHORT", "wshort_k5", 2, "k_wgrad_short"),
    ("W_32", "c32_l64", 2, "k_wgrad32"), ("W_K5_pre", "w5_l7", 2, "k_wgrad_k5_pre"), ("W_K5_split", "w5_l12_split", 2, "k_wgrad_k5_split"),
    ("W_ROWS", "wrows_l9", 2, "k_wgrad_rows"), ("W_ROWS3", "wrows3_l4096", 2, "k_wgrad_rows3"), ("W_MFMA", "mfma_m48", 2, "k_igemm_wgrad"),
    ("W_G4", "g4x4_l65", 2, "k_g4_wgrad"), ("W_G3", "g4_l260", 2, "k_gconv_split_wgrad"), ("W_DIRECT", "judge_l17", 2, "k_conv1d_bwd_weight_direct"),
    ("W_DIRECT_s2", "direct_s2", 2, "k_conv1d_bwd_weight_direct"),
]
for _route, _shape, _which, _stem_ in CONV_ROUTES:
    case("conv_%s" % _route, _CONV_SYMS[_which], conv_case, _S[_shape], _which, _stem_, None, "exact", None,
         3 if "PAD4" in _route else 0)
# W_G (gconv_mfma.hip: split slabs + slab reduce) stands behind W_G3 for every geometry it takes: reached with the split-bf16
# grouped kernels switched off, as tests/test_gpu_ops.py does for its generation-against-generation test
_S["g16_lrelu"] = ("mc_g16_lrelu", 2, 64, 64, 256, 41, 4, 20, 1, 16, 1, False)
case("conv_W_G", "ms_conv1d_bwd_weight", conv_case, _S["g16_lrelu"], 2, "k_gconv_mfma_wgrad", None, "exact", None, 0, MS_OK, None,
     {"MSYNTH_GCONV3": "0"})
case("conv_W_G_g4_long", "ms_conv1d_bwd_weight", conv_case, ("mc_g4_l1025", 2, 16, 1025, 64, 41, 4, 20, 1, 4, 1, False), 2,
     "k_gconv_mfma_wgrad", None, "exact", None, 0, MS_OK, None, {"MSYNTH_GCONV3": "0"})
# Lin <= 2 pad + 1: mirrored taps of both edges meet on one sample (the only case compared at a tolerance: ATOMIC_ROUTES)
case("conv_D_DIRECT_reflect_fold_colliding", "ms_conv1d_bwd_data", conv_case, ("mc_reflect_l6", 2, 24, 6, 160, 7, 1, 3, 1, 1, 2, True), 1,
     "k_conv1d_bwd_data_direct")

# (b) every declining route declined.  Each operand below is one its launcher TESTS before anything is launched
# (wgrad_rows.hip msw_conv1d_bwd_weight / msw32_bwd_weight, wgrad_short.hip msws_bwd_weight: x / gy / y_act -> MS_ERR_UNSUPPORTED),
# and the route behind them, W_MFMA, picks its dword kernel and dword reduce from the same pointers (conv_mfma.hip
# msm_conv1d_bwd_weight, msm_wgrad_reduce); the padded-row routes are skipped by the plan itself on a short or 4-byte
# workspace, and F_MFMA / D_MFMA behind them test the workspace before they use it.
for _route, _shape, _stem_, _ops in (("W_ROWS", "wrows_l9", "k_wgrad_rows", ("x", "gy", "y_act")),
                                     ("W_32", "c32_l64", "k_wgrad32", ("x", "gy", "y_act")),
                                     ("W_SHORT", "wshort_k5", "k_wgrad_short", ("gy", "y_act"))):
    for _op in _ops:
        # (W_ROWS takes short tiles with its dword loader instead of declining: no other stem is required of it)
        case("conv_%s_declines_%s_plus4" % (_route, _op), "ms_conv1d_bwd_weight", conv_case, _S[_shape], 2, None, {_op: 4}, "exact",
             None if _route == "W_ROWS" else _stem_)
# W_MFMA itself with the gradient outputs and the workspace at 4-byte addresses: the dword reduce (msm_wgrad_reduce tests both)
case("conv_W_MFMA_gw_gb_ws_plus4", "ms_conv1d_bwd_weight", conv_case, _S["mfma_m48"], 2, None, {"gw": 4, "gb": 4}, "plus4")
for _w in (0, 1):
    case("conv_%s_PAD4_declines_ws_plus4" % "FD"[_w], _CONV_SYMS[_w], conv_case, _S["k5_l17_pad4"], _w, None, None, "plus4")
    case("conv_%s_PAD4_declines_null_ws" % "FD"[_w], _CONV_SYMS[_w], conv_case, _S["k5_l17_pad4"], _w, None, None, "null")
# (every weight-gradient route of this layer sums split-K slabs: without a workspace the call is refused, nothing written)
case("conv_W_K5_declines_null_ws", "ms_conv1d_bwd_weight", conv_case, _S["w5_l7"], 2, None, None, "null", None, 0, MS_ERR_WORKSPACE)
# the last routes of every plan are plain dword kernels (conv_direct.hip has no vector access): any placement
for _w in (0, 1, 2):
    case("conv_%s_DIRECT_all_plus4" % "FDW"[_w], _CONV_SYMS[_w], conv_case, _S["direct_s2"], _w, None,
         {"x": 4, "w": 4, "y": 4, "y_act": 4, "residual": 8, "gy": 4, "gx": 12, "gx_add": 8, "gw": 4, "gb": 4}, "plus4")
# F_MFMA with the weights at a 4-byte address: the row kernels read them 16 bytes at a time and are not taken
# (conv_mfma.hip plan_fwd tests w), the im2col kernel behind reads dwords
case("conv_F_MFMA_declines_w_plus4", "ms_conv1d_fwd", conv_case, _S["mfma_m48"], 0, None, {"w": 4})


# launchers that pick their 16-byte or dword form from the operand's address (gconv_split.hip: vec / vout; conv_thin.hip: vec;
# wgrad_k5.hip: vec): each operand below is one of those the launcher tests, on a shape whose aligned call takes the 16-byte form
_S["g3_vec_l512"] = ("mc_g3_vec_l512", 2, 16, 512, 64, 41, 4, 20, 1, 4, 1, False)
_S["thin_l1024"] = ("mc_thin_l1024", 2, 32, 1024, 1, 7, 1, 3, 1, 1, 2, False)
_S["k15_l1024"] = ("mc_k15_l1024", 2, 1, 1024, 16, 15, 1, 7, 1, 1, 1, False)
for _nm, _shape, _which, _ops in (("F_G3", "g3_vec_l512", 0, ("x", "y")), ("D_G3", "g3_vec_l512", 1, ("gy", "y_act", "gx", "gx_add")),
                                  ("W_G3", "g3_vec_l512", 2, ("x", "gy", "y_act")),
                                  ("F_THIN", "thin_l1024", 0, ("x",)), ("D_THIN", "thin_l1024", 1, ("gx", "gx_add")),
                                  ("W_THIN", "thin_l1024", 2, ("x",)), ("D_THIN_k15", "k15_l1024", 1, ("gy", "y_act")),
                                  ("W_THIN_k15", "k15_l1024", 2, ("gy", "y_act")), ("W_K5_split", "w5_l12_split", 2, ("x", "gy"))):
    # the grouped split-bf16 launchers and the k5 split launcher record the form they took: <.., vec, vout> / <vec, vout> / <vec>;
    # the thin launchers record none (the note is the route's), there the values and the clean arena are the check
    _al = {"F_G3": r"<\d+, true, true>", "D_G3": r"<true, true>", "W_G3": r"<true>", "W_K5_split": r"k5_split<true>"}.get(_nm)
    case("conv_%s_aligned_form" % _nm, _CONV_SYMS[_which], conv_case, _S[_shape], _which, None, None, "exact", None, 0, MS_OK, _al)
    for _op in _ops:
        _dw = {"F_G3": {"x": r"<\d+, false, true>", "y": r"<\d+, true, false>"},
               "D_G3": {"gy": r"<false, true>", "y_act": r"<false, true>", "gx": r"<true, false>", "gx_add": r"<true, false>"},
               "W_G3": {"x": r"<false>", "gy": r"<false>", "y_act": r"<false>"},
               "W_K5_split": {"x": r"k5_split<false>", "gy": r"k5_split<false>"}}.get(_nm, {}).get(_op)
        case("conv_%s_dword_form_%s_plus4" % (_nm, _op), _CONV_SYMS[_which], conv_case, _S[_shape], _which, None, {_op: 4}, "exact",
             None, 0, MS_OK, _dw)
# the row-tile routes F_MFMA / D_MFMA pick the pipelined kernels only for 16-byte operands (conv_mfma.hip plan_rows tests x, w,
# y, y_act, residual); behind them k_conv_mfma_rows reads and writes these tensors as dwords.
for _op in ("x", "y", "y_act", "residual"):
    case("conv_F_MFMA_rows_%s_plus4" % _op, "ms_conv1d_fwd", conv_case, _S["k3_l16_rows"], 0, None, {_op: 4})
for _op in ("gy", "y_act", "gx", "gx_add"):
    case("conv_D_MFMA_rows_%s_plus4" % _op, "ms_conv1d_bwd_data", conv_case, _S["k3_l16_rows"], 1, None, {_op: 4})


def convt_case(shape, which, stem=None, offs=None, ws_mode="exact", differs=None, expect=MS_OK):
    """ms_convt1d_fwd / _bwd_data (with and without y_act) / _bwd_weight (beta 0 and 1, with gb); as conv_case."""
    from oracle import oracle as O
    L, lib = _L()
    s = L.stream()
    offs = offs or {}
    name, B, Cin, Lg, Cout, K, st, pad = shape
    r = np.random.default_rng(stable_seed(name))
    x = r.standard_normal((B, Cin, Lg)).astype(np.float32)
    w = (r.standard_normal((Cin, Cout, K)) * 0.1).astype(np.float32)
    b = (r.standard_normal((Cout,)) * 0.1).astype(np.float32)
    d = L.ConvTDesc(B, Cin, Lg, Cout, K, st, pad, 1, SLOPE, 0)
    Lo = lib.ms_convt1d_out_len(d)
    ya = O.conv_transpose1d_fwd(x, w, b, st, pad, O.ACT_LRELU).astype(np.float32)
    assert ya.shape == (B, Cout, Lo)
    gy = r.standard_normal(ya.shape).astype(np.float32)
    gw0 = r.standard_normal(w.shape).astype(np.float32)
    gb0 = r.standard_normal(b.shape).astype(np.float32)
    query = lib.ms_convt1d_kernel_name(d, which).decode()
    nws = lib.ms_convt1d_workspace_bytes(d, which)
    floats = 2 * x.size + 3 * ya.size + 3 * w.size + nws // 4 + 64
    o = lambda k: offs.get(k, 0)
    T = torch.from_numpy
    for variant in ((0,) if which == 0 else (0, 1)):
        a = arena(floats)
        notes = []
        if which == 0:
            xb, wb, bb = a.put(T(x), name="x", offset_bytes=o("x")), a.put(T(w), name="w", offset_bytes=o("w")), a.put(T(b), name="bias")
            yb = a.take(ya.shape, "output", name="y", offset_bytes=o("y"))
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_convt1d_fwd(d, xb.ptr, wb.ptr, bb.ptr, yb.ptr, wsp, wsn, s)
        elif which == 1:
            gyb, wb = a.put(T(gy), name="gy", offset_bytes=o("gy")), a.put(T(w), name="w", offset_bytes=o("w"))
            yab = a.put(T(ya), name="y_act", offset_bytes=o("y_act")) if variant == 0 else None
            gxb = a.take(x.shape, "output", name="gx", offset_bytes=o("gx"))
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_convt1d_bwd_data(d, gyb.ptr, ptr(yab), wb.ptr, gxb.ptr, wsp, wsn, s)
        else:
            xb, gyb = a.put(T(x), name="x", offset_bytes=o("x")), a.put(T(gy), name="gy", offset_bytes=o("gy"))
            yab = a.put(T(ya), name="y_act", offset_bytes=o("y_act"))
            if variant:
                gwb, gbb = a.put(T(gw0), "accumulate", name="gw", offset_bytes=o("gw")), a.put(T(gb0), "accumulate", name="gb")
            else:
                gwb, gbb = a.take(w.shape, "output", name="gw", offset_bytes=o("gw")), a.take(b.shape, "output", name="gb")
            wsb, wsp, wsn = _workspace(a, nws, ws_mode)
            call = lambda: lib.ms_convt1d_bwd_weight(d, xb.ptr, gyb.ptr, yab.ptr, gwb.ptr, gbb.ptr, float(variant), wsp, wsn, s)
        rc, out = a.run_twice(profiled(call, notes), sync)
        plain = not offs and ws_mode == "exact"
        assert rc == expect, "status %d, expected %d (%s)" % (rc, expect, notes)
        if rc != MS_OK:
            continue
        if variant == 0 and plain:
            # (the bias sum behind a weight gradient notes nothing: the note is the route's)
            assert _stem(notes[0][0]) == _stem(query), (notes, query)
            if stem:
                assert _stem(query) == stem, (query, stem)
        if variant == 0 and differs:
            assert _stem(notes[0][0]) != differs, "the declined route's kernel ran: %s" % (notes,)
        if variant == 0 and stem and not plain:
            assert _stem(notes[0][0]) == stem, "expected the route behind the declining one: %s" % (notes,)
        if which == 0:
            assert rel_l2(cpu(out["y"]), ya) < FWD_TOL
        elif which == 1:
            gp = O.act_bwd(ya, gy, O.ACT_LRELU) if variant == 0 else gy
            assert rel_l2(cpu(out["gx"]), O.conv_transpose1d_bwd_data(gp, w, x.shape, st, pad)) < GRAD_TOL
        else:
            gp = O.act_bwd(ya, gy, O.ACT_LRELU)
            gw_ref, gb_ref = O.conv_transpose1d_bwd_weight(x, gp, w.shape, st, pad)
            assert rel_l2(cpu(out["gw"]), gw_ref.astype(np.float64) + (gw0 if variant else 0)) < GRAD_TOL
            assert rel_l2(cpu(out["gb"]), gb_ref.astype(np.float64) + (gb0 if variant else 0)) < GRAD_TOL


_CONVT_SYMS = ("ms_convt1d_fwd", "ms_convt1d_bwd_data", "ms_convt1d_bwd_weight")
# name, B, Cin, L, Cout, K, stride, pad (the layout of HOT_CONVT)
_T = {
    "thin_l131": ("ct_thin_c40_l131", 3, 40, 131, 1, 4, 2, 1),
    "lanes_s8": ("mc_ct_lanes_s8", 3, 20, 65, 6, 16, 8, 4),
    "w8_l32": ("ct_w8_l32", 3, 128, 32, 48, 16, 8, 4),
    "rows_s8_b32": ("mc_ct_rows_s8", 32, 128, 36, 48, 16, 8, 4),
    "direct": ("mc_ct_direct", 2, 6, 11, 5, 4, 2, 1),
    "s2_small": ("mc_ct_s2_small", 2, 32, 16, 8, 4, 2, 1),
    "s1_k3_c32": ("mc_ct_s1_k3_c32", 2, 32, 40, 16, 3, 1, 1),
    "s1_k3": ("mc_ct_s1_k3", 2, 16, 40, 16, 3, 1, 1),
    "t2s": ("mc_ct_t2s", 32, 128, 8, 64, 4, 2, 1),
    "s2_128_64": ("ct_128_64", 2, 128, 130, 64, 4, 2, 1),
}
CONVT_ROUTES = [
    ("TF_THIN", "thin_l131", 0, "k_convt1_fwd"), ("TF_LANES", "lanes_s8", 0, "k_convt_lanes"), ("TF_MFMA", "rows_s8_b32", 0, "k_conv_rows2"),
    ("TF_DIRECT", "direct", 0, "k_conv1d_bwd_data_direct"),
    ("TD_MFMA", "s2_small", 1, "k_conv_rows2"), ("TD_MFMA_s8", "w8_l32", 1, "k_conv_rows2"), ("TD_CONV_MFMA", "s1_k3_c32", 1, "k_conv_mfma_rows"),
    ("TD_CONV_DIRECT", "direct", 1, "k_conv1d_fwd_direct"), ("TD_CONV_DIRECT_thin", "thin_l131", 1, "k_conv1d_fwd_direct"),
    ("TW_THIN", "thin_l131", 2, "k_convt1_wgrad"), ("TW_8", "w8_l32", 2, "k_wgrad_convt8_split"), ("TW_2S", "t2s", 2, "k_wgrad_convt2_short"),
    ("TW_MFMA", "s2_128_64", 2, "k_igemm_wgrad"), ("TW_CONV_MFMA", "s1_k3", 2, "k_igemm_wgrad_v4"),
    ("TW_CONV_DIRECT", "direct", 2, "k_conv1d_bwd_weight_direct"),
]
for _route, _shape, _which, _stem_ in CONVT_ROUTES:
    case("convt_%s" % _route, _CONVT_SYMS[_which], convt_case, _T[_shape], _which, _stem_)


# (b) TF_LANES tests w (small_rows.hip mss_convt_fwd) and passes the call on to TF_MFMA, whose pack kernel reads w as dwords;
# TF_MFMA tests y (its phase-interleaved epilogue stores 8 / 16 bytes) and passes it on to the dword kernel TF_DIRECT;
# TW_8 / TW_2S test x, gy, y_act (wgrad_convt.hip, wgrad_convt2s.hip) before any launch.
case("convt_TF_LANES_declines_w_plus4", "ms_convt1d_fwd", convt_case, _T["w8_l32"], 0, None, {"w": 4}, "exact", "k_convt_lanes")
case("convt_TF_MFMA_declines_y_plus4", "ms_convt1d_fwd", convt_case, _T["rows_s8_b32"], 0, "k_conv1d_bwd_data_direct", {"y": 4}, "exact",
     "k_conv_mfma_rows")
case("convt_TF_MFMA_s2_declines_y_plus4", "ms_convt1d_fwd", convt_case, ("mc_ct_rows_s2", 8, 64, 1028, 32, 4, 2, 1), 0,
     "k_conv1d_bwd_data_direct", {"y": 8}, "exact", "k_conv_mfma_rows")
for _route, _shape in (("TW_8", "w8_l32"), ("TW_2S", "t2s")):
    for _op in ("x", "gy", "y_act"):
        case("convt_%s_declines_%s_plus4" % (_route, _op), "ms_convt1d_bwd_weight", convt_case, _T[_shape], 2, None, {_op: 4})
# TD_MFMA behind plan_rows: k_conv_mfma_rows reads the phase-split gradient and writes gx as dwords
for _op in ("gy", "y_act", "gx"):
    case("convt_TD_MFMA_rows_%s_plus4" % _op, "ms_convt1d_bwd_data", convt_case, _T["s2_small"], 1, None, {_op: 4})
case("convt_DIRECT_all_plus4", _CONVT_SYMS, lambda: [convt_case(_T["direct"], wh, None, {"x": 4, "w": 4, "y": 4, "gy": 4, "y_act": 8,
                                                                                      "gx": 12, "gw": 4}, "plus4") for wh in (0, 1, 2)])
case("convt_null_workspace_refused", "ms_convt1d_fwd", convt_case, _T["rows_s8_b32"], 0, None, None, "null", None, MS_ERR_WORKSPACE)

# ================================================================ (c) fused and image kernels

def _d64(t):
    return t.cuda().double()


def _lrelu_mask(y):
    return torch.where(y > 0, 1.0, SLOPE).double()


def _image(a, nbytes, name, role="output", off=0):
    assert nbytes % 4 == 0
    # (an image buffer is sized for the larger of the two piece schemes; a pack writes what the active scheme reads, and the
    #  kernels are handed the NaN-poisoned copy: a read of the unwritten part shows in their values)
    return a.take((nbytes // 4,), role, name=name, offset_bytes=off, partial=True)


def atom_case(shape):
    """ms_residual_atom_pack_multi (weights at 4-byte addresses: its kernels read them through aligned(4) vectors and dwords),
    _fwd (training and inference), _fwd_signs, _bwd_data, _bwd_data_signs; then every operand the header wants 16-byte aligned
    moved by 4 bytes: MS_ERR_INVALID_ARG and nothing written."""
    from oracle import torch_graph as TG
    from test_gpu_atom import _inputs
    L, lib = _L()
    s = L.stream()
    name, B, C, Lg, dil = shape
    x, w0, b0, w1, b1 = (torch.from_numpy(v) for v in _inputs(name, B, C, Lg))
    d = L.AtomDesc(B, C, Lg, dil, SLOPE)
    assert lib.ms_residual_atom_supported(d) and lib.ms_residual_atom_bwd_supported(d)
    nimg, nsign = lib.ms_residual_atom_image_bytes(C), lib.ms_residual_atom_sign_words(d)
    amax_n = 2 * L.ATOM_AMAX_N if lib.ms_residual_atom_publishes_amax() else 0
    n = x.numel()
    # ---- pack: both images in one call
    a = arena(2 * w0.numel() + 3 * nimg // 4 + 64)
    w0b, w1b = a.put(w0, name="w0", offset_bytes=4), a.put(w1, name="w1", offset_bytes=12)
    imf, imb = _image(a, nimg, "image_fwd"), _image(a, nimg, "image_bwd")
    pd = L.AtomPackDesc()
    pd.count = 2
    for k, im in enumerate((imf, imb)):
        pd.C[k], pd.w0[k], pd.w1[k], pd.image[k], pd.backward[k] = C, w0b.ptr, w1b.ptr, im.ptr, k
    rc, packed = a.run_twice(lambda: lib.ms_residual_atom_pack_multi(pd, s), sync)
    assert rc == MS_OK
    bad = _image(a, nimg, "image_plus4", off=4)
    pd.image[1] = bad.ptr
    rc, _ = a.run_twice(lambda: lib.ms_residual_atom_pack_multi(pd, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    # ---- forward: training, inference, sign words
    a = arena(12 * n + nimg // 2 + 4 * amax_n + 4 * C + nsign + 64, nbuf=32)
    xb, imf = a.put(x, name="x"), a.put(packed["image_fwd"], name="image_fwd")
    b0b, b1b = a.put(b0, name="b0"), a.put(b1, name="b1")
    b0x = a.put(b0, name="b0_plus4", offset_bytes=4)
    yb, tb, ub = (a.take(x.shape, "output", name=k) for k in ("y", "t", "y_act"))
    yi = a.take(x.shape, "output", name="y_inference")
    am = a.take((amax_n,), "output", name="amax") if amax_n else None
    rc, out = a.run_twice(lambda: lib.ms_residual_atom_fwd(d, xb.ptr, imf.ptr, b0b.ptr, b1b.ptr, yb.ptr, tb.ptr, ub.ptr, ptr(am), s) or
                          lib.ms_residual_atom_fwd(d, xb.ptr, imf.ptr, b0b.ptr, b1b.ptr, yi.ptr, None, None, None, s), sync)
    assert rc == MS_OK
    x64 = _d64(x)
    t64 = TF.leaky_relu(TF.conv1d(x64, _d64(w0), _d64(b0), padding=dil, dilation=dil), SLOPE)
    u64 = TF.leaky_relu(TF.conv1d(t64, _d64(w1), _d64(b1), padding=1), SLOPE)
    for k, ref in (("y", x64 + u64), ("t", t64), ("y_act", u64), ("y_inference", x64 + u64)):
        assert rel_l2(cpu(out[k]), cpu(ref)) < 1e-5, k                       # (tests/test_gpu_atom.py's oracle gate)
    assert torch.equal(out["y"], out["y_inference"])
    t_dev, u_dev = out["t"], out["y_act"]
    rc, _ = a.run_twice(lambda: lib.ms_residual_atom_fwd(d, xb.ptr, imf.ptr, b0x.ptr, b1b.ptr, yb.ptr, tb.ptr, ub.ptr, ptr(am), s), sync)
    assert rc == MS_ERR_INVALID_ARG
    rc, _ = a.run_twice(lambda: lib.ms_residual_atom_fwd(d, xb.ptr, imf.ptr, b0b.ptr, b0x.ptr, yb.ptr, tb.ptr, ub.ptr, ptr(am), s), sync)
    assert rc == MS_ERR_INVALID_ARG
    signs = None
    if nsign:
        a2 = arena(3 * n + nimg // 4 + 2 * amax_n + 2 * C + 3 * nsign + 64)
        xb, imf = a2.put(x, name="x"), a2.put(packed["image_fwd"], name="image_fwd")
        b0b, b1b = a2.put(b0, name="b0"), a2.put(b1, name="b1")
        yb, tb = a2.take(x.shape, "output", name="y"), a2.take(x.shape, "output", name="t")
        ts_ = a2.take((nsign // 2,), "output", name="t_signs", dtype=torch.int32)
        ys_ = a2.take((nsign // 2,), "output", name="y_signs", dtype=torch.int32)
        am = a2.take((amax_n,), "output", name="amax")
        rc, signs = a2.run_twice(lambda: lib.ms_residual_atom_fwd_signs(d, xb.ptr, imf.ptr, b0b.ptr, b1b.ptr, yb.ptr, tb.ptr, ts_.ptr,
                                                                       ys_.ptr, am.ptr, s), sync)
        assert rc == MS_OK
        assert torch.equal(signs["y"], out["y"]) and torch.equal(signs["t"], t_dev)
        for k, act in (("t_signs", t_dev), ("y_signs", u_dev)):
            words = signs[k].view(torch.int16).view(B, C // 32, 2, Lg)
            assert torch.equal(TG.decode_sign_words(words.cpu()).to(act.device), act > 0), k
        ysx = a2.take((nsign // 2,), "output", name="y_signs_plus4", dtype=torch.int32, offset_bytes=4)
        rc, _ = a2.run_twice(lambda: lib.ms_residual_atom_fwd_signs(d, xb.ptr, imf.ptr, b0b.ptr, b1b.ptr, yb.ptr, tb.ptr, ts_.ptr,
                                                                   ysx.ptr, am.ptr, s), sync)
        assert rc == MS_ERR_INVALID_ARG
    # ---- backward data
    g = rnd(name + "g", B, C, Lg)
    a3 = arena(8 * n + nimg // 4 + 4 * amax_n + 2 * nsign + 64)
    gb_, ub, tb = a3.put(g, name="gy"), a3.put(u_dev, name="y_act", offset_bytes=0), a3.put(t_dev, name="t")
    imb = a3.put(packed["image_bwd"], name="image_bwd")
    gtb, gxb = a3.take(x.shape, "output", name="gt"), a3.take(x.shape, "output", name="gx")
    am = a3.take((amax_n,), "output", name="amax") if amax_n else None
    calls = [lambda: lib.ms_residual_atom_bwd_data(d, gb_.ptr, ub.ptr, tb.ptr, imb.ptr, gtb.ptr, gxb.ptr, ptr(am), s)]
    if nsign:
        tsb, ysb = a3.put(signs["t_signs"], name="t_signs"), a3.put(signs["y_signs"], name="y_signs")
        tsx = a3.put(signs["t_signs"], name="t_signs_plus4", offset_bytes=4)
        gts, gxs = a3.take(x.shape, "output", name="gt_signs"), a3.take(x.shape, "output", name="gx_signs")
        am2 = a3.take((amax_n,), "output", name="amax_signs")
        calls.append(lambda: lib.ms_residual_atom_bwd_data_signs(d, gb_.ptr, ysb.ptr, tsb.ptr, imb.ptr, gts.ptr, gxs.ptr, am2.ptr, s))
    rc, out = a3.run_twice(lambda: calls[0]() or (calls[1]() if nsign else 0), sync)
    assert rc == MS_OK
    gt64 = TF.conv_transpose1d(_d64(g) * _lrelu_mask(u_dev), _d64(w1), padding=1)
    gx64 = _d64(g) + TF.conv_transpose1d(gt64 * _lrelu_mask(t_dev), _d64(w0), padding=dil, dilation=dil)
    assert rel_l2(cpu(out["gt"]), cpu(gt64)) < 1e-5 and rel_l2(cpu(out["gx"]), cpu(gx64)) < 1e-5
    if nsign:
        assert torch.equal(out["gt_signs"], out["gt"]) and torch.equal(out["gx_signs"], out["gx"])
        rc, _ = a3.run_twice(lambda: lib.ms_residual_atom_bwd_data_signs(d, gb_.ptr, ysb.ptr, tsx.ptr, imb.ptr, gts.ptr, gxs.ptr,
                                                                        am2.ptr, s), sync)
        assert rc == MS_ERR_INVALID_ARG


_ATOM_SYMS = ("ms_residual_atom_pack_multi", "ms_residual_atom_fwd", "ms_residual_atom_fwd_signs", "ms_residual_atom_bwd_data",
              "ms_residual_atom_bwd_data_signs")
# one aligned and one ragged case per channel count (tests/test_gpu_atom.py: ATOM_CASES)
for _c in (("c32_d1_one_tile", 1, 32, 124, 1), ("c32_d9_ragged", 2, 32, 1032, 9), ("c64_d3_two_rows", 2, 64, 248, 3),
           ("c64_d9_tail4", 1, 64, 252, 9), ("c128_d3", 2, 128, 64, 3), ("c128_d9_ragged", 1, 128, 188, 9),
           ("c256_d1_b1", 1, 256, 256, 1), ("c256_d9_ragged", 2, 256, 100, 9)):
    case("atom_%s" % _c[0], _ATOM_SYMS, atom_case, _c)


def stack_case(B, C, Lg, dils):
    from test_gpu_atom import _inputs
    L, lib = _L()
    s = L.stream()
    d = L.StackDesc()
    d.B, d.C, d.L, d.count, d.slope = B, C, Lg, len(dils), SLOPE
    for i, dl in enumerate(dils):
        d.dil[i] = dl
    assert lib.ms_residual_stack_supported(d)
    nimg = lib.ms_residual_atom_image_bytes(C)
    x = rnd("stack%d%d" % (C, Lg), B, C, Lg)
    a = arena(3 * x.numel() + len(dils) * (nimg // 2 + 6 * C * C + 4 * C) + 64, nbuf=40)
    pd = L.AtomPackDesc()
    pd.count = len(dils)
    ws_, ims = [], []
    for k in range(len(dils)):
        _, w0, b0, w1, b1 = (torch.from_numpy(v) for v in _inputs("stack%d_%d" % (C, k), 1, C, 8))
        ws_.append((w0, b0, w1, b1))
        im = _image(a, nimg, "image%d" % k)
        ims.append(im)
        pd.C[k], pd.w0[k], pd.w1[k], pd.image[k], pd.backward[k] = C, a.put(w0, name="w0_%d" % k, offset_bytes=4).ptr, \
            a.put(w1, name="w1_%d" % k).ptr, im.ptr, 0
    rc, packed = a.run_twice(lambda: lib.ms_residual_atom_pack_multi(pd, s), sync)
    assert rc == MS_OK
    a = arena(3 * x.numel() + len(dils) * (nimg // 4 + 4 * C) + 64, nbuf=40)
    xb, yb = a.put(x, name="x"), a.take(x.shape, "output", name="y")
    imb = [a.put(packed["image%d" % k], name="image%d" % k) for k in range(len(dils))]
    b0b = [a.put(ws_[k][1], name="b0_%d" % k) for k in range(len(dils))]
    b1b = [a.put(ws_[k][3], name="b1_%d" % k) for k in range(len(dils))]
    b1x = a.put(ws_[0][3], name="b1_plus4", offset_bytes=4)
    arr = ctypes.c_void_p * len(dils)
    pim, pb0, pb1 = arr(*[b.ptr for b in imb]), arr(*[b.ptr for b in b0b]), arr(*[b.ptr for b in b1b])
    pbx = arr(*([b1x.ptr] + [b.ptr for b in b1b[1:]]))
    cv = lambda p: ctypes.cast(p, ctypes.c_void_p)
    rc, out = a.run_twice(lambda: lib.ms_residual_stack_fwd(d, xb.ptr, cv(pim), cv(pb0), cv(pb1), yb.ptr, s), sync)
    assert rc == MS_OK
    h = _d64(x)
    for (w0, b0, w1, b1), dl in zip(ws_, dils):
        t = TF.leaky_relu(TF.conv1d(h, _d64(w0), _d64(b0), padding=dl, dilation=dl), SLOPE)
        h = h + TF.leaky_relu(TF.conv1d(t, _d64(w1), _d64(b1), padding=1), SLOPE)
    assert rel_l2(cpu(out["y"]), cpu(h)) < 1e-5                              # (tests/test_gpu_stack.py's oracle gate)
    rc, _ = a.run_twice(lambda: lib.ms_residual_stack_fwd(d, xb.ptr, cv(pim), cv(pb0), cv(pbx), yb.ptr, s), sync)
    assert rc == MS_ERR_INVALID_ARG


case("stack_c32_ragged", ("ms_residual_stack_fwd", "ms_residual_atom_pack_multi"), stack_case, 2, 32, 1000, (1, 3, 9))
case("stack_c64_tiny", ("ms_residual_stack_fwd", "ms_residual_atom_pack_multi"), stack_case, 3, 64, 8, (1, 3, 9))


def _conv_ref64(x, w, b, st, pad, g, act):
    pre = TF.conv1d(_d64(x), _d64(w), _d64(b) if b is not None else None, stride=st, padding=pad, groups=g)
    return TF.leaky_relu(pre, SLOPE) if act else pre


def conv5_img_case(shape):
    """ms_conv1d_img_pack / _pack2 (weights at a 4-byte address: dword reads), _img_fwd, _img_bwd_data with and without gx_add,
    exact workspaces; image / bias at 4-byte addresses: MS_ERR_INVALID_ARG."""
    L, lib = _L()
    s = L.stream()
    name, B, Cin, Cout, Lg, act = shape
    x, w, b = rnd(name, B, Cin, Lg), rnd(name + "w", Cout, Cin, 5, scale=1.0 / np.sqrt(5 * Cin)), rnd(name + "b", Cout, scale=0.1)
    d = L.ConvDesc(B, Cin, Lg, Cout, 5, 1, 2, 1, 1, 0, act, SLOPE, 0)
    nimg = lib.ms_conv1d_img_bytes(d)
    assert nimg > 0
    a = arena(w.numel() + 5 * nimg // 4 + 64)
    wb = a.put(w, name="w", offset_bytes=4)
    ims = [_image(a, nimg, k) for k in ("fwd", "bwd", "fwd2", "bwd2")]
    rc, packed = a.run_twice(lambda: lib.ms_conv1d_img_pack(d, wb.ptr, 0, ims[0].ptr, s) or lib.ms_conv1d_img_pack(d, wb.ptr, 1, ims[1].ptr, s) or
                             lib.ms_conv1d_img_pack2(d, wb.ptr, ims[2].ptr, ims[3].ptr, s), sync)
    assert rc == MS_OK
    imx = _image(a, nimg, "image_plus4", off=4)
    for c in (lambda: lib.ms_conv1d_img_pack(d, wb.ptr, 0, imx.ptr, s), lambda: lib.ms_conv1d_img_pack2(d, wb.ptr, ims[2].ptr, imx.ptr, s)):
        rc, _ = a.run_twice(c, sync)
        assert rc == MS_ERR_INVALID_ARG
    y64 = _conv_ref64(x, w, b, 1, 2, 1, act)
    ya = y64.float().cpu()
    gy, add = rnd(name + "gy", *ya.shape), rnd(name + "add", *x.shape)
    n0, n1 = lib.ms_conv1d_img_workspace_bytes(d, 0), lib.ms_conv1d_img_workspace_bytes(d, 1)
    a = arena(4 * x.numel() + 4 * ya.numel() + nimg + (n0 + n1) // 4 + 64)
    xb, bb, bx = a.put(x, name="x"), a.put(b, name="bias"), a.put(b, name="bias_plus4", offset_bytes=4)
    imf, imb = a.put(packed["fwd"], name="image_fwd"), a.put(packed["bwd2"], name="image_bwd")
    yb = a.take(ya.shape, "output", name="y")
    gyb, yab, addb = a.put(gy, name="gy"), (a.put(ya, name="y_act") if act else None), a.put(add, name="gx_add")
    gx0, gx1 = a.take(x.shape, "output", name="gx"), a.take(x.shape, "output", name="gx_added")
    w0, w0p, w0n = _workspace(a, n0, "exact")
    w1 = a.take(n1, "workspace", name="ws_bwd") if n1 else None
    rc, out = a.run_twice(lambda: lib.ms_conv1d_img_fwd(d, xb.ptr, imf.ptr, bb.ptr, yb.ptr, w0p, w0n, s) or
                          lib.ms_conv1d_img_bwd_data(d, gyb.ptr, ptr(yab), imb.ptr, None, gx0.ptr, ptr(w1), n1, s) or
                          lib.ms_conv1d_img_bwd_data(d, gyb.ptr, ptr(yab), imb.ptr, addb.ptr, gx1.ptr, ptr(w1), n1, s), sync)
    assert rc == MS_OK
    assert rel_l2(cpu(out["y"]), cpu(y64)) < 1e-5                           # (tests/test_gpu_conv5.py's oracle gates)
    gp = _d64(gy) * (_lrelu_mask(ya.cuda()) if act else 1.0)
    gx64 = TF.conv_transpose1d(gp, _d64(w), padding=2)
    assert rel_l2(cpu(out["gx"]), cpu(gx64)) < 1e-5 and rel_l2(cpu(out["gx_added"]), cpu(gx64 + _d64(add))) < 1e-5
    rc, _ = a.run_twice(lambda: lib.ms_conv1d_img_fwd(d, xb.ptr, imf.ptr, bx.ptr, yb.ptr, w0p, w0n, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    imx = a.put(packed["fwd"], name="image_plus4", offset_bytes=4)
    for c in (lambda: lib.ms_conv1d_img_fwd(d, xb.ptr, imx.ptr, bb.ptr, yb.ptr, w0p, w0n, s),
              lambda: lib.ms_conv1d_img_bwd_data(d, gyb.ptr, ptr(yab), imx.ptr, None, gx0.ptr, ptr(w1), n1, s)):
        rc, _ = a.run_twice(c, sync)
        assert rc == MS_ERR_INVALID_ARG


_C5 = ("ms_conv1d_img_pack", "ms_conv1d_img_pack2", "ms_conv1d_img_fwd", "ms_conv1d_img_bwd_data")
for _c in (("l32_b3", 3, 256, 320, 32, 1), ("l17_b5", 5, 320, 256, 17, 1), ("l9_b64", 64, 256, 256, 9, 0), ("l32_b64_split", 64, 256, 256, 32, 1)):
    case("conv5_img_%s" % _c[0], _C5, conv5_img_case, _c)


def convt_img_case(shape):
    """ms_convt1d_img_pack / _img_fwd (convt_img.hip, and convt_fwd_short.hip on short rows) with the exact workspace."""
    L, lib = _L()
    s = L.stream()
    name, B, Cin, Lin, Cout, S, act = shape
    K, pad = 2 * S, S // 2
    x, w, b = rnd(name, B, Cin, Lin), rnd(name + "w", Cin, Cout, K, scale=1.0 / np.sqrt(2 * Cin)), rnd(name + "b", Cout, scale=0.1)
    d = L.ConvTDesc(B, Cin, Lin, Cout, K, S, pad, act, SLOPE, 0)
    nimg, nws = lib.ms_convt1d_img_bytes(d), lib.ms_convt1d_img_workspace_bytes(d)
    assert nimg > 0
    a = arena(w.numel() + 3 * nimg // 4 + 64)
    wb, im = a.put(w, name="w", offset_bytes=4), _image(a, nimg, "image")
    rc, packed = a.run_twice(lambda: lib.ms_convt1d_img_pack(d, wb.ptr, im.ptr, s), sync)
    assert rc == MS_OK
    imx = _image(a, nimg, "image_plus4", off=4)
    rc, _ = a.run_twice(lambda: lib.ms_convt1d_img_pack(d, wb.ptr, imx.ptr, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    Lo = lib.ms_convt1d_out_len(d)
    a = arena(x.numel() + B * Cout * Lo + 3 * nimg // 4 + nws // 4 + 64)
    xb, bb, imb = a.put(x, name="x"), a.put(b, name="bias"), a.put(packed["image"], name="image")
    imx = a.put(packed["image"], name="image_plus4", offset_bytes=4)
    yb = a.take((B, Cout, Lo), "output", name="y")
    wsb, wsp, wsn = _workspace(a, nws, "exact")
    rc, out = a.run_twice(lambda: lib.ms_convt1d_img_fwd(d, xb.ptr, imb.ptr, bb.ptr, yb.ptr, wsp, wsn, s), sync)
    assert rc == MS_OK
    y64 = TF.conv_transpose1d(_d64(x), _d64(w), _d64(b), stride=S, padding=pad)
    y64 = TF.leaky_relu(y64, SLOPE) if act else y64
    assert rel_l2(cpu(out["y"]), cpu(y64)) < 1e-5                           # (tests/test_gpu_convt_img.py's gate)
    rc, _ = a.run_twice(lambda: lib.ms_convt1d_img_fwd(d, xb.ptr, imx.ptr, bb.ptr, yb.ptr, wsp, wsn, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    if nws:
        rc, _ = a.run_twice(lambda: lib.ms_convt1d_img_fwd(d, xb.ptr, imb.ptr, bb.ptr, yb.ptr, wsp, wsn - 16, s), sync)
        assert rc == MS_ERR_WORKSPACE


for _c in (("l2_b5_ragged_noact", 5, 256, 212, 128, 8, 0), ("l1_b40_ragged", 40, 512, 28, 256, 8, 1),
           ("short_w16_noact", 40, 256, 16, 128, 2, 0), ("short_w8_ragged", 130, 1024, 8, 256, 2, 1)):
    case("convt_img_%s" % _c[0], ("ms_convt1d_img_pack", "ms_convt1d_img_fwd"), convt_img_case, _c)


def convt_bwd_img_case(shape):
    """ms_convt1d_bwd_img_pack / _bwd_img_data with the exact split-K workspace; image / gx at 4-byte addresses are refused."""
    L, lib = _L()
    s = L.stream()
    name, B, Cin, Lin, Cout, S, act = shape
    K, pad = 2 * S, S // 2
    w = rnd(name + "w", Cin, Cout, K, scale=1.0 / np.sqrt(2 * Cout))
    gy, ya = rnd(name + "gy", B, Cout, Lin * S), rnd(name + "y", B, Cout, Lin * S)
    d = L.ConvTDesc(B, Cin, Lin, Cout, K, S, pad, act, SLOPE, 0)
    nimg, nws = lib.ms_convt1d_bwd_img_bytes(d), lib.ms_convt1d_bwd_img_workspace_bytes(d)
    assert nimg > 0
    a = arena(w.numel() + 3 * nimg // 4 + 64)
    wb, im = a.put(w, name="w", offset_bytes=4), _image(a, nimg, "image")
    rc, packed = a.run_twice(lambda: lib.ms_convt1d_bwd_img_pack(d, wb.ptr, im.ptr, s), sync)
    assert rc == MS_OK
    imx = _image(a, nimg, "image_plus4", off=4)
    rc, _ = a.run_twice(lambda: lib.ms_convt1d_bwd_img_pack(d, wb.ptr, imx.ptr, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    a = arena(2 * gy.numel() + 2 * B * Cin * Lin + nimg // 4 + nws // 4 + 64)
    gyb, yab, imb = a.put(gy, name="gy"), (a.put(ya, name="y_act") if act else None), a.put(packed["image"], name="image")
    gxb = a.take((B, Cin, Lin), "output", name="gx")
    wsb, wsp, wsn = _workspace(a, nws, "exact")
    rc, out = a.run_twice(lambda: lib.ms_convt1d_bwd_img_data(d, gyb.ptr, ptr(yab), imb.ptr, gxb.ptr, wsp, wsn, s), sync)
    assert rc == MS_OK
    gxx = a.take((B, Cin, Lin), "output", name="gx_plus4", offset_bytes=4)
    g64 = _d64(gy) * (_lrelu_mask(ya.cuda()) if act else 1.0)
    ref = TF.conv1d(g64, _d64(w), None, S, pad)
    assert rel_l2(cpu(out["gx"]), cpu(ref)) < 1e-5                          # (tests/test_gpu_convt_img.py's gate)
    rc, _ = a.run_twice(lambda: lib.ms_convt1d_bwd_img_data(d, gyb.ptr, ptr(yab), imb.ptr, gxx.ptr, wsp, wsn, s), sync)
    assert rc == MS_ERR_INVALID_ARG
    if nws:
        rc, _ = a.run_twice(lambda: lib.ms_convt1d_bwd_img_data(d, gyb.ptr, ptr(yab), imb.ptr, gxb.ptr, wsp, wsn - 16, s), sync)
        assert rc == MS_ERR_WORKSPACE


for _c in (("g2_b8", 8, 256, 256, 128, 8, 1), ("s1_w8_ragged", 130, 1024, 8, 256, 2, 1), ("s1_w64_noact", 16, 256, 64, 64, 2, 0),
           ("s1_w128_m192", 9, 192, 128, 32, 2, 1)):
    case("convt_bwd_img_%s" % _c[0], ("ms_convt1d_bwd_img_pack", "ms_convt1d_bwd_img_data"), convt_bwd_img_case, _c)


# ================================================================ (d) one layer over several inputs

def parts_case(kind, geo, B, lens, act, stems, image=False, off_part=None, each=False):
    """ms_conv1d_parts_fwd / _bwd_data / _bwd_weight over three parts, each with guarded buffers of its own.  stems: the kernels
    the three calls must note (the parts kind the case exists for); off_part = (part, byte offset): that part's tensors sit at a
    4-byte address and the call must still be right (the plan goes part by part) or refuse."""
    L, lib = _L()
    s = L.stream()
    Cin, Cout, K, st, pad, g = geo
    d = L.ConvDesc(B, Cin, lens[0], Cout, K, st, pad, 1, g, 0, act, SLOPE, 0)
    w = rnd(kind + "w", Cout, Cin // g, K, scale=1.0 / np.sqrt(K * Cin // g))
    b = rnd(kind + "b", Cout, scale=0.1)
    xs = [rnd("%sx%d" % (kind, i), B, Cin, l) for i, l in enumerate(lens)]
    y64 = [_conv_ref64(x, w, b, st, pad, g, act) for x in xs]
    yas = [y.float().cpu() for y in y64]
    gys = [rnd("%sgy%d" % (kind, i), *y.shape) for i, y in enumerate(yas)]
    adds = [rnd("%sadd%d" % (kind, i), *x.shape) for i, x in enumerate(xs)]
    o = lambda i: off_part[1] if off_part and off_part[0] == i else 0
    nx, ny = sum(x.numel() for x in xs), sum(y.numel() for y in yas)
    packed = None
    if image:
        nimg = lib.ms_conv1d_img_bytes(d)
        assert nimg > 0
        a = arena(w.numel() + nimg // 2 + 64)
        wb, imf, imb = a.put(w, name="w"), _image(a, nimg, "image_fwd"), _image(a, nimg, "image_bwd")
        rc, packed = a.run_twice(lambda: lib.ms_conv1d_img_pack2(d, wb.ptr, imf.ptr, imb.ptr, s), sync)
        assert rc == MS_OK

    def table(a, which):
        p = L.ConvParts()
        p.count = len(lens)
        bufs = {}
        for i, l in enumerate(lens):
            p.B[i], p.Lin[i] = B, l
            if which in (0, 2):
                bufs["x%d" % i] = a.put(xs[i], name="x%d" % i, offset_bytes=o(i))
                p.x[i] = bufs["x%d" % i].ptr
            if which == 0:
                p.y[i] = a.take(yas[i].shape, "output", name="y%d" % i, offset_bytes=o(i)).ptr
            if which in (1, 2):
                p.gy[i] = a.put(gys[i], name="gy%d" % i, offset_bytes=o(i)).ptr
                p.y_act[i] = a.put(yas[i], name="y_act%d" % i, offset_bytes=o(i)).ptr if act else None
            if which == 1:
                p.gx_add[i] = a.put(adds[i], name="gx_add%d" % i, offset_bytes=o(i)).ptr
                p.gx[i] = a.take(xs[i].shape, "output", name="gx%d" % i, offset_bytes=o(i)).ptr
        return p

    for which in (0, 1, 2):
        if image and which == 2:
            continue
        for beta in ((0, 1) if which == 2 else (0,)):
            a = arena(3 * nx + 4 * ny + 3 * w.numel() + (lib.ms_conv1d_img_bytes(d) // 4 if image else 0) + (96 << 20) // 4, nbuf=40)
            p = table(a, which)
            nws = lib.ms_conv1d_parts_workspace_bytes(d, p, which, 1 if image else 0)
            launches = lib.ms_conv1d_parts_launches(d, p, which, 1 if image else 0)
            wb, bb = a.put(w, name="w"), a.put(b, name="bias")
            im = a.put(packed["image_bwd" if which else "image_fwd"], name="image") if image else None
            wsb, wsp, wsn = _workspace(a, nws, "exact")
            notes = []
            if which == 0:
                call = lambda: lib.ms_conv1d_parts_fwd(d, p, wb.ptr, bb.ptr, ptr(im), wsp, wsn, s)
            elif which == 1:
                call = lambda: lib.ms_conv1d_parts_bwd_data(d, p, wb.ptr, ptr(im), wsp, wsn, s)
            else:
                gw0, gb0 = rnd(kind + "gw0", *w.shape), rnd(kind + "gb0", *b.shape)
                gwb = a.put(gw0, "accumulate", name="gw") if beta else a.take(w.shape, "output", name="gw")
                gbb = a.put(gb0, "accumulate", name="gb") if beta else a.take(b.shape, "output", name="gb")
                call = lambda: lib.ms_conv1d_parts_bwd_weight(d, p, gwb.ptr, gbb.ptr, float(beta), wsp, wsn, s)
            rc, out = a.run_twice(profiled(call, notes), sync)
            if off_part:
                assert rc == MS_OK, rc          # (part by part ends in routes that take any placement)
                assert launches == len(lens), "a part at a 4-byte address goes part by part"
            else:
                assert rc == MS_OK
                assert launches == (len(lens) if (each[which] if isinstance(each, tuple) else each) else 1), (which, launches)
                if stems and stems[which]:
                    assert _stem(notes[0][0]).startswith(stems[which]), (which, notes)
            if which == 0:
                for i in range(len(lens)):
                    assert rel_l2(cpu(out["y%d" % i]), cpu(y64[i])) < FWD_TOL, i
            elif which == 1:
                for i in range(len(lens)):
                    gp = _d64(gys[i]) * (_lrelu_mask(yas[i].cuda()) if act else 1.0)
                    ref = TF.conv_transpose1d(gp, _d64(w), stride=st, padding=pad, groups=g,
                                              output_padding=lens[i] - ((yas[i].shape[2] - 1) * st - 2 * pad + K))
                    assert rel_l2(cpu(out["gx%d" % i]), cpu(ref + _d64(adds[i]))) < GRAD_TOL, i
            else:
                wd = _d64(w).requires_grad_(True)
                bd = _d64(b).requires_grad_(True)
                tot = 0
                for i in range(len(lens)):
                    gp = _d64(gys[i]) * (_lrelu_mask(yas[i].cuda()) if act else 1.0)
                    tot = tot + (TF.conv1d(_d64(xs[i]), wd, bd, stride=st, padding=pad, groups=g) * gp).sum()
                gwr, gbr = torch.autograd.grad(tot, (wd, bd))
                assert rel_l2(cpu(out["gw"]), cpu(gwr + (_d64(gw0) if beta else 0))) < GRAD_TOL
                assert rel_l2(cpu(out["gb"]), cpu(gbr + (_d64(gb0) if beta else 0))) < GRAD_TOL


_PARTS = ("ms_conv1d_parts_fwd", "ms_conv1d_parts_bwd_data", "ms_conv1d_parts_bwd_weight")
# the discriminator's 8192 / 4097 / 2049 ladder, shortened to what still reaches each parts kind (api.hip: P_*)
case("parts_P_DISC_first", _PARTS, parts_case, "pd_first", (1, 16, 15, 1, 7, 1), 2, (512, 257, 129), 1,
     ("k_dfirst_fwd", "k_dfirst_bwd_data", "k_dfirst_wgrad"))
case("parts_P_DISC_judge", _PARTS, parts_case, "pd_judge", (1024, 1, 3, 1, 1, 1), 2, (32, 17, 9), 0,
     ("k_djudge_fwd", "k_djudge_bwd_data", "k_djudge_wgrad"))
case("parts_P_G4", _PARTS, parts_case, "pg4", (1024, 1024, 41, 4, 20, 256), 1, (29, 65, 33), 1, ("k_g4_fwd", "k_g4_bwd_data", "k_g4_wgrad"))
case("parts_P_G3", _PARTS, parts_case, "pg3", (256, 1024, 41, 4, 20, 64), 1, (512, 257, 129), 1,
     ("k_gconv_split_fwd_parts", "k_gconv_split_bwd_data_parts", "k_gconv_split_wgrad_parts"))
# (forward and backward data of this layer go part by part without an image; its weight gradient is one launch over the parts)
case("parts_P_K5", "ms_conv1d_parts_bwd_weight", parts_case, "pk5", (256, 256, 5, 1, 2, 1), 2, (32, 17, 9), 1,
     (None, None, "k_wgrad_k5_"), False, None, (True, True, False))
case("parts_P_K5_IMG", ("ms_conv1d_parts_fwd", "ms_conv1d_parts_bwd_data", "ms_conv1d_img_pack2"), parts_case, "pk5img",
     (1024, 1024, 5, 1, 2, 1), 32, (32, 17, 9), 1, ("k_conv5_img_parts", "k_conv5_img_parts", None), True)
case("parts_P_EACH", _PARTS, parts_case, "peach", (16, 64, 41, 4, 20, 4), 2, (300, 151, 76), 1, None, False, None, True)
# one part at a 4-byte address: the judge conv's parts kernels load 16 bytes at a time (disc_parts.hip msd_parts_applicable tests
# x / gx / gx_add) -> part by part on the thin kernels, which pick their dword forms from the same pointers (conv_thin.hip)
case("parts_P_DISC_judge_part1_plus4", _PARTS, parts_case, "pd_judge4", (1024, 1, 3, 1, 1, 1), 2, (32, 17, 9), 0, None, False, (1, 4))

def wgrad_multi_case(B, C, Lg, dils, betas, off_entry=None):
    """ms_conv1d_bwd_weight_multi with the exact workspace of its query; off_entry: that entry's x at a 4-byte address -- the batched
    launchers test every pointer (wgrad_rows.hip) and the call falls back entry by entry."""
    L, lib = _L()
    s = L.stream()
    n = len(dils)
    md = L.WgradMultiDesc()
    md.count = n
    a = arena(n * (3 * B * C * Lg + 2 * 3 * C * C + 2 * C) + (64 << 20) // 4, nbuf=8 * n + 4)
    refs = []
    for i, (dil, beta) in enumerate(zip(dils, betas)):
        x, gy, ya = (rnd("wm%s%d%d" % (k, C, i), B, C, Lg) for k in "xgy")
        gw0, gb0 = rnd("wmgw%d%d" % (C, i), C, C, 3), rnd("wmgb%d%d" % (C, i), C)
        md.conv[i] = L.ConvDesc(B, C, Lg, C, 3, 1, dil, dil, 1, 0, 1, SLOPE, 0)
        md.x[i] = a.put(x, name="x%d" % i, offset_bytes=4 if off_entry == i else 0).ptr
        md.gy[i], md.y_act[i] = a.put(gy, name="gy%d" % i).ptr, a.put(ya, name="y_act%d" % i).ptr
        md.gw[i] = (a.put(gw0, "accumulate", name="gw%d" % i) if beta else a.take((C, C, 3), "output", name="gw%d" % i)).ptr
        md.gb[i] = (a.put(gb0, "accumulate", name="gb%d" % i) if beta else a.take((C,), "output", name="gb%d" % i)).ptr
        md.beta[i] = float(beta)
        wd, bd = torch.zeros(C, C, 3, dtype=torch.float64, device="cuda", requires_grad=True), \
            torch.zeros(C, dtype=torch.float64, device="cuda", requires_grad=True)
        gp = _d64(gy) * _lrelu_mask(ya.cuda())
        gwr, gbr = torch.autograd.grad((TF.conv1d(_d64(x), wd, bd, padding=dil, dilation=dil) * gp).sum(), (wd, bd))
        refs.append((gwr + (_d64(gw0) if beta else 0), gbr + (_d64(gb0) if beta else 0)))
    nws = lib.ms_conv1d_bwd_weight_multi_workspace_bytes(md)
    wsb, wsp, wsn = _workspace(a, nws, "exact")
    notes = []
    rc, out = a.run_twice(profiled(lambda: lib.ms_conv1d_bwd_weight_multi(md, wsp, wsn, s), notes), sync)
    assert rc == MS_OK
    if off_entry is None:
        assert notes[0][1] <= 3, "one batched launch pair, not entry by entry: %s" % (notes,)
    else:
        assert notes[0][1] >= n, "entry by entry: %s" % (notes,)
    for i, (gwr, gbr) in enumerate(refs):
        assert rel_l2(cpu(out["gw%d" % i]), cpu(gwr)) < GRAD_TOL and rel_l2(cpu(out["gb%d" % i]), cpu(gbr)) < GRAD_TOL, i


case("wgrad_multi_c64", "ms_conv1d_bwd_weight_multi", wgrad_multi_case, 2, 64, 256, (1, 9, 1, 3), (0, 1, 0, 0))
case("wgrad_multi_c32", "ms_conv1d_bwd_weight_multi", wgrad_multi_case, 2, 32, 512, (1, 3, 9, 1), (0, 1, 0, 0))
case("wgrad_multi_c64_entry1_plus4", "ms_conv1d_bwd_weight_multi", wgrad_multi_case, 2, 64, 256, (1, 9, 1, 3), (0, 1, 0, 0), 1)


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_memory_contract(c):
    c.fn(*c.args)
