"""The kernel-name queries against the dispatch (run with -m gpu on an MI355X): every conv and transposed-conv layer and
pass of the bench workloads is called once in a profile session, without residual / fused y_act output, and the kernel
the call noted is the one ms_conv1d_kernel_name / ms_convt1d_kernel_name names: the whole string, template arguments
included, for the row-tile family of conv_mfma.hip (query and launcher read one plan and share one formatter per kernel
template); the stem (the text before '<') for the other families."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _layers():
    from featuresynth import _workload as W
    convs, convts = [], []      # (name, B, Cin, Lin, Cout, K, stride, pad, dil, groups, pad_mode, act) / ConvTDesc fields
    for B in (32, 1):
        L = 32
        convs.append(("g.first", B, 80, L, 512, 7, 1, 3, 1, 1, 1, 1))
        for cin, cout, k, s, p in W.G_UPS:
            convts.append(("g.convT%d" % cout, B, cin, L, cout, k, s, p, 1))
            L = (L - 1) * s - 2 * p + k
            for d in (1, 3, 9):
                convs.append(("atom%d.d%d" % (cout, d), B, cout, L, cout, 3, 1, d, d, 1, 0, 1))
        convs.append(("g.last", B, 32, L, 1, 7, 1, 3, 1, 1, 1, 2))
        for L0 in (8192, 4097, 2049):
            l = L0
            for i, (cin, cout, k, st, p, g) in enumerate(W.D_MAIN):
                convs.append(("d.main%d.L%d" % (i, L0), B, cin, l, cout, k, st, p, 1, g, 0, 1))
                l = W.conv_out_len(l, k, st, p)
            convs.append(("d.judge.L%d" % L0, B, 1024, l, 1, 3, 1, 1, 1, 1, 0, 0))
    return convs, convts


CONVS, CONVTS = _layers()


# kernels of the msm_* routes (conv_mfma.hip, conv_rows2.hip, conv_rows3.hip): their launchers note the instantiation
MSM_STEMS = ("k_conv_rows3p", "k_conv_rows3", "k_conv_rows2", "k_conv_mfma_rows", "k_igemm_conv", "k_igemm_wgrad", "k_igemm_wgrad_v4")


def _stem(name):
    return name.split("<")[0].strip()


def _same_kernel(noted, query):
    if _stem(query) in MSM_STEMS:
        return noted == query
    return _stem(noted) == _stem(query)


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


def _t(*shape):
    return torch.randn(*shape, device="cuda", dtype=torch.float32)


@pytest.mark.parametrize("layer", CONVS, ids=lambda c: "%s.B%d" % (c[0], c[1]))
def test_conv_kernel_name_is_what_runs(layer):
    from featuresynth._ops import lib as L
    _, B, Cin, Lin, Cout, K, st, pad, dil, g, pm, act = layer
    d = L.ConvDesc(B, Cin, Lin, Cout, K, st, pad, dil, g, pm, act, 0.2, 0)
    lib = L.load()
    Lout = lib.ms_conv1d_out_len(d)
    x, w, b = _t(B, Cin, Lin), _t(Cout, Cin // g, K) * 0.05, _t(Cout)
    y, gy = _t(B, Cout, Lout), _t(B, Cout, Lout)
    ya = y if act else None
    gx, gw, gb = _t(B, Cin, Lin), _t(Cout, Cin // g, K), _t(Cout)
    s = L.stream()
    for which in (0, 1, 2):
        query = lib.ms_conv1d_kernel_name(d, which).decode()
        nws = lib.ms_conv1d_workspace_bytes(d, which)
        ws = L.workspace(nws, "cuda")
        if which == 0:
            call = lambda: lib.ms_conv1d_fwd(d, x.data_ptr(), w.data_ptr(), b.data_ptr(), None, y.data_ptr(), None,
                                             L.ptr(ws), nws, s)
        elif which == 1:
            if not query:            # (no backward data: a strided / grouped reflection-padded conv)
                continue
            call = lambda: lib.ms_conv1d_bwd_data(d, gy.data_ptr(), L.ptr(ya), w.data_ptr(), None, gx.data_ptr(),
                                                  L.ptr(ws), nws, s)
        else:
            call = lambda: lib.ms_conv1d_bwd_weight(d, x.data_ptr(), gy.data_ptr(), L.ptr(ya), gw.data_ptr(),
                                                    gb.data_ptr(), 0.0, L.ptr(ws), nws, s)
        noted = _noted(L, call)
        assert _same_kernel(noted, query), (which, noted, query)
    torch.cuda.synchronize()


@pytest.mark.parametrize("layer", CONVTS, ids=lambda c: "%s.B%d" % (c[0], c[1]))
def test_convt_kernel_name_is_what_runs(layer):
    from featuresynth._ops import lib as L
    _, B, Cin, Lin, Cout, K, st, pad, act = layer
    d = L.ConvTDesc(B, Cin, Lin, Cout, K, st, pad, act, 0.2, 0)
    lib = L.load()
    Lout = lib.ms_convt1d_out_len(d)
    x, w, b = _t(B, Cin, Lin), _t(Cin, Cout, K) * 0.05, _t(Cout)
    y, gy = _t(B, Cout, Lout), _t(B, Cout, Lout)
    gx, gw, gb = _t(B, Cin, Lin), _t(Cin, Cout, K), _t(Cout)
    s = L.stream()
    for which in (0, 1, 2):
        query = lib.ms_convt1d_kernel_name(d, which).decode()
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
