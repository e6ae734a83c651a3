"""ConvTranspose1d(k = 8, stride 4, padding 2) -- the LearnedUpSample layers of the multi-scale band generator -- on the
phase-split matrix-pipe kernels (run with -m gpu on an MI355X): parity of the three passes against the CPU oracle at
lengths the pipelined kernels take and at lengths that fall through, the paired split-bf16 forward against float64, and
the routes: the generator's own shapes leave the direct kernels in every pass, the name query names what runs, and
MSYNTH_CONVT_S4=0 gives the direct kernels back.

Tolerances are those of tests/test_gpu_ops.py (single op, fp32 accumulation order only)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_l2, stable_seed

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD_TOL = 1e-5
GRAD_TOL = 1e-4
K, S, PAD = 8, 4, 2

# (name, B, Cin, Lin, Cout)
PIPELINED = [("s4_512_256_l32", 3, 512, 32, 256), ("s4_256_128_l132", 1, 256, 132, 128),
             ("s4_128_64_l192", 2, 128, 192, 64), ("s4_64_32_l1028", 1, 64, 1028, 32)]
FALL_THROUGH = [("s4_512_256_l9", 2, 512, 9, 256), ("s4_256_128_l70", 1, 256, 70, 128),
                ("s4_128_64_l130", 2, 128, 130, 64), ("s4_64_32_l1027", 1, 64, 1027, 32)]
# the generator's stride-4 layers of the 8192 band at the training batch
GENERATOR = [(32, 512, 32, 256), (32, 256, 128, 128), (32, 128, 512, 64), (32, 64, 2048, 32)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def _operands(name, B, Cin, L, Cout):
    rng = np.random.default_rng(stable_seed(name))
    x = rng.standard_normal((B, Cin, L)).astype(np.float32)
    w = (rng.standard_normal((Cin, Cout, K)) * 0.1).astype(np.float32)
    b = (rng.standard_normal((Cout,)) * 0.1).astype(np.float32)
    return rng, x, w, b


@pytest.mark.parametrize("case", PIPELINED + FALL_THROUGH, ids=[c[0] for c in PIPELINED + FALL_THROUGH])
def test_convt_s4_vs_oracle(case):
    """forward + LeakyReLU, backward data, weight and bias gradients"""
    from featuresynth._ops import functional as F_
    from oracle import oracle as O
    name, B, Cin, L, Cout = case
    rng, x, w, b = _operands(name, B, Cin, L, Cout)
    y_ref = O.conv_transpose1d_fwd(x, w, b, S, PAD, O.ACT_LRELU)
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    xt, wt, bt = dev(x).requires_grad_(True), dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    y = F_.ConvTranspose1dFn.apply(xt, wt, bt, S, PAD, 1)
    assert rel_l2(host(y), y_ref) < FWD_TOL
    gp = O.act_bwd(host(y), gy, O.ACT_LRELU)      # mask from the device's activations
    gx, gw, gb = torch.autograd.grad(y, (xt, wt, bt), dev(gy))
    assert rel_l2(host(gx), O.conv_transpose1d_bwd_data(gp, w, x.shape, S, PAD)) < GRAD_TOL
    gw_ref, gb_ref = O.conv_transpose1d_bwd_weight(x, gp, w.shape, S, PAD)
    assert rel_l2(host(gw), gw_ref) < GRAD_TOL
    assert rel_l2(host(gb), gb_ref) < GRAD_TOL


@pytest.mark.parametrize("case", [PIPELINED[0], PIPELINED[2], FALL_THROUGH[1]], ids=lambda c: c[0])
def test_convt_s4_without_bias(case):
    """LearnedUpSample's own form: bias=False, LeakyReLU behind"""
    from featuresynth._ops import functional as F_
    from oracle import oracle as O
    name, B, Cin, L, Cout = case
    rng, x, w, _ = _operands(name + "nobias", B, Cin, L, Cout)
    y_ref = O.conv_transpose1d_fwd(x, w, None, S, PAD, O.ACT_LRELU)
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    xt, wt = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
    y = F_.ConvTranspose1dFn.apply(xt, wt, None, S, PAD, 1)
    assert rel_l2(host(y), y_ref) < FWD_TOL
    gp = O.act_bwd(host(y), gy, O.ACT_LRELU)
    gx, gw = torch.autograd.grad(y, (xt, wt), dev(gy))
    assert rel_l2(host(gx), O.conv_transpose1d_bwd_data(gp, w, x.shape, S, PAD)) < GRAD_TOL
    assert rel_l2(host(gw), O.conv_transpose1d_bwd_weight(x, gp, w.shape, S, PAD)[0]) < GRAD_TOL


@pytest.mark.parametrize("case", [PIPELINED[1], PIPELINED[3], FALL_THROUGH[2]], ids=lambda c: c[0])
def test_convt_s4_with_activation_in_front(case):
    """in_act = 1: y = conv_transpose1d(lrelu(x)) + bias, no activation behind; the gradients of x pass through lrelu'"""
    from featuresynth._ops import functional as F_
    from oracle import oracle as O
    name, B, Cin, L, Cout = case
    rng, x, w, b = _operands(name + "inact", B, Cin, L, Cout)
    xa = np.where(x > 0, x, np.float32(0.2) * x).astype(np.float32)
    y_ref = O.conv_transpose1d_fwd(xa, w, b, S, PAD, O.ACT_NONE)
    gy = rng.standard_normal(y_ref.shape).astype(np.float32)
    xt, wt, bt = dev(x).requires_grad_(True), dev(w).requires_grad_(True), dev(b).requires_grad_(True)
    y = F_.ConvTranspose1dExFn.apply(xt, wt, bt, S, PAD, 0, 1)
    assert rel_l2(host(y), y_ref) < FWD_TOL
    gx, gw, gb = torch.autograd.grad(y, (xt, wt, bt), dev(gy))
    gxa = O.conv_transpose1d_bwd_data(gy, w, x.shape, S, PAD)
    assert rel_l2(host(gx), np.where(x > 0, gxa, np.float32(0.2) * gxa)) < GRAD_TOL
    gw_ref, gb_ref = O.conv_transpose1d_bwd_weight(xa, gy, w.shape, S, PAD)
    assert rel_l2(host(gw), gw_ref) < GRAD_TOL
    assert rel_l2(host(gb), gb_ref) < GRAD_TOL


@pytest.mark.parametrize("shape", [(32, 512, 36, 256), (16, 128, 516, 64)], ids=["packed_rows_m1024", "tail_m256"])
@pytest.mark.parametrize("in_act", [0, 1])
def test_convt_s4_paired_split_kernel(shape, in_act):
    """The forward on the paired split-bf16 kernel (conv_rows3.hip, two-tap form: >= 128 workgroups) against float64: rows
    packed 3 per tile and a column-tile tail, 128- and 64-row workgroups, with and without the LeakyReLU in front."""
    import torch.nn.functional as TF
    from featuresynth._ops import prims as P
    B, Cin, Lin, Cout = shape
    g = torch.Generator(device="cuda").manual_seed(stable_seed("convt3s4%s%d" % (shape, in_act)) % (1 << 31))
    x = torch.randn(B, Cin, Lin, device="cuda", generator=g)
    w = torch.randn(Cin, Cout, K, device="cuda", generator=g) * 0.05
    b = torch.randn(Cout, device="cuda", generator=g)
    d, lo = P.convt_desc(x.shape, w.shape, S, PAD, act=1, in_act=in_act)
    name = P.L.load().ms_convt1d_kernel_name(d, 0).decode()
    assert "k_conv_rows3p" in name and ", 4, " in name, name
    y = torch.full((B, Cout, lo), float("nan"), device="cuda")            # every output element must be written
    P.convt1d_fwd(x, w, b, d, lo, out=y)
    xin = TF.leaky_relu(x.double(), 0.2) if in_act else x.double()
    ref = TF.leaky_relu(TF.conv_transpose1d(xin, w.double(), b.double(), stride=S, padding=PAD), 0.2)
    assert tuple(y.shape) == tuple(ref.shape)
    assert float((y.double() - ref).norm() / ref.norm()) < 1e-6


@pytest.mark.parametrize("shape, tile", [((16, 40, 1028, 32), "1, 4, 2, 1"), ((32, 40, 1536, 32), "2, 2, 2, 2")],
                         ids=["64x128_tail", "128x128"])
@pytest.mark.parametrize("in_act", [0, 1])
def test_convt_s4_two_tap_fp32_kernel(shape, tile, in_act):
    """The forward on the fp32-MFMA two-tap kernel (conv_rows2.hip, [low | high] phase rows; 40 input channels keep the
    split-bf16 kernel, which takes chunks of 16, away) against float64: both of its tiles, a column-tile tail, with and
    without the LeakyReLU in front.  fp32 products and sums: 1e-6."""
    import torch.nn.functional as TF
    from featuresynth._ops import prims as P
    B, Cin, Lin, Cout = shape
    g = torch.Generator(device="cuda").manual_seed(stable_seed("convt2s4%s%d" % (shape, in_act)) % (1 << 31))
    x = torch.randn(B, Cin, Lin, device="cuda", generator=g)
    w = torch.randn(Cin, Cout, K, device="cuda", generator=g) * 0.05
    b = torch.randn(Cout, device="cuda", generator=g)
    d, lo = P.convt_desc(x.shape, w.shape, S, PAD, act=1, in_act=in_act)
    name = P.L.load().ms_convt1d_kernel_name(d, 0).decode()
    assert name == "k_conv_rows2<%s, 2, 8, %d, 4, 1>" % (tile, 3 if in_act else 0), name
    y = torch.full((B, Cout, lo), float("nan"), device="cuda")            # every output element must be written
    P.convt1d_fwd(x, w, b, d, lo, out=y)
    xin = TF.leaky_relu(x.double(), 0.2) if in_act else x.double()
    ref = TF.leaky_relu(TF.conv_transpose1d(xin, w.double(), b.double(), stride=S, padding=PAD), 0.2)
    assert tuple(y.shape) == tuple(ref.shape)
    assert float((y.double() - ref).norm() / ref.norm()) < 1e-6


MSM_STEMS = ("k_conv_rows3p", "k_conv_rows3", "k_conv_rows2", "k_conv_mfma_rows", "k_igemm_conv", "k_igemm_wgrad", "k_igemm_wgrad_v4")


def _same_kernel(noted, query):
    if query.split("<")[0].strip() in MSM_STEMS:
        return noted == query
    return noted.split("<")[0].strip() == query.split("<")[0].strip()


def _noted(L, call):
    rec = L.ProfileRecord()
    L.load().ms_profile_take(ctypes.byref(rec))
    L.load().ms_profile_kernels(1)
    try:
        rc = call()
        L.load().ms_profile_take(ctypes.byref(rec))
    finally:
        L.load().ms_profile_kernels(0)
    L.check(rc, "profiled call")
    return rec.kernel.decode()


@pytest.mark.parametrize("shape", GENERATOR, ids=lambda s: "c%d_l%d" % (s[1], s[2]))
def test_generator_shapes_leave_the_direct_kernels(shape):
    """all three passes of the generator's stride-4 layers at B = 32 run the matrix-pipe routes, and a profile session
    notes the kernel the query names"""
    from featuresynth._ops import lib as L
    B, Cin, Lin, Cout = shape
    d = L.ConvTDesc(B, Cin, Lin, Cout, K, S, PAD, 1, 0.2, 0)
    lib = L.load()
    Lout = lib.ms_convt1d_out_len(d)
    t = lambda *s: torch.randn(*s, device="cuda", dtype=torch.float32)
    x, w, b = t(B, Cin, Lin), t(Cin, Cout, K) * 0.05, t(Cout)
    y, gy = t(B, Cout, Lout), t(B, Cout, Lout)
    gx, gw, gb = t(B, Cin, Lin), t(Cin, Cout, K), t(Cout)
    s = L.stream()
    for which in (0, 1, 2):
        query = lib.ms_convt1d_kernel_name(d, which).decode()
        assert query and "_direct" not in query, (which, query)
        nws = lib.ms_convt1d_workspace_bytes(d, which)
        ws = L.workspace(nws, "cuda")
        if which == 0:
            call = lambda: lib.ms_convt1d_fwd(d, x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), L.ptr(ws), nws, s)
        elif which == 1:
            call = lambda: lib.ms_convt1d_bwd_data(d, gy.data_ptr(), y.data_ptr(), w.data_ptr(), gx.data_ptr(), L.ptr(ws),
                                                   nws, s)
        else:
            call = lambda: lib.ms_convt1d_bwd_weight(d, x.data_ptr(), gy.data_ptr(), y.data_ptr(), gw.data_ptr(),
                                                     gb.data_ptr(), 0.0, L.ptr(ws), nws, s)
        noted = _noted(L, call)
        assert _same_kernel(noted, query), (which, noted, query)
    torch.cuda.synchronize()


_CHILD = r"""
import sys
from featuresynth._ops import lib as L
lib = L.load()
for B, Cin, Lin, Cout in %r:
    d = L.ConvTDesc(B, Cin, Lin, Cout, 8, 4, 2, 1, 0.2, 0)
    print(" | ".join(lib.ms_convt1d_kernel_name(d, which).decode() for which in (0, 1, 2)))
"""


def test_switch_off_gives_the_direct_kernels_back():
    """MSYNTH_CONVT_S4=0 (read in a fresh process): the three predicates refuse S = 4 and the direct kernels run"""
    env = dict(os.environ, MSYNTH_CONVT_S4="0")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "music-synthesis_amd")] +
                                        ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    out = subprocess.check_output([sys.executable, "-c", _CHILD % (GENERATOR,)], env=env, text=True, timeout=120)
    lines = [ln for ln in out.splitlines() if " | " in ln]
    assert len(lines) == len(GENERATOR)
    for ln in lines:
        fwd, bwd, wgrad = ln.split(" | ")
        assert fwd.startswith("k_conv1d_bwd_data_direct"), ln       # (a transposed conv's forward is a conv's backward data)
        assert bwd.startswith("k_conv1d_fwd_direct"), ln
        assert wgrad.startswith("k_conv1d_bwd_weight_direct"), ln
