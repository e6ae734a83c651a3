"""featuresynth.audio on the device (run with -m gpu on an MI355X): the band split, the merge, fft_resample and their
gradients (csrc/bands.hip) against the float64 restatement of the reference (tests/bands_ref.py), MultiScale and the
Experiment hooks.

Tolerance.  Every result is compared with the float64 restatement; the gate is GATE x e32, where e32 is the error of the
SAME restatement run in float32 with stock torch.fft on the CPU, on the same input and against the same float64 values.
The factor covers a radix-2 LDS transform with ~log2 N rounding steps and sincospif twiddles, where the stock FFT uses
higher radices and tabulated twiddles.  Both numbers are in every assert message.

Measured on an MI355X (HIP / stock float32, worst band; DESIGN.md "Band split / merge" has every shape): N = 8192 split
2.19e-7 / 1.96e-7, merge 1.98e-7 / 1.71e-7; N = 32768 split 2.35e-7 / 2.20e-7, merge gradient 2.34e-7 / 2.15e-7; the worst
ratio of any case is 1.43.
"""
import ctypes

import numpy as np
import pytest

import bands_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GATE = 8.0
# (N, min_size, (B, C)): odd row count with C > 1 and the smallest bands; one band (lowest-only path); the training
# shape; the largest LDS configuration
SHAPES = [(256, 16, (3, 2)), (64, 64, (2, 1)), (8192, 512, (2, 1)), (32768, 2048, (1, 1))]


def T():
    from featuresynth.audio import transform
    return transform


def rnd(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def held(got, want64, ref32, what):
    assert tuple(got.shape) == tuple(want64.shape), (what, tuple(got.shape), tuple(want64.shape))
    assert got.dtype == torch.float32 and got.is_cuda, what
    e, e32 = rel_l2(got.detach().cpu().numpy(), want64.detach().numpy()), rel_l2(ref32.detach().numpy(), want64.detach().numpy())
    print("%-44s HIP %.3e  stock float32 %.3e  ratio %.2f" % (what, e, e32, e / e32))
    assert e <= GATE * e32, "%s: %.3e against the float64 restatement, stock float32 %.3e (gate %gx)" % (what, e, e32, GATE)


_REF = {}


def reference(N, m, lead):
    """Inputs, cotangents and the float64 / float32 restatement results of one shape: computed once, never changed."""
    key = (N, m, lead)
    if key in _REF:
        return _REF[key]
    sizes = R.band_sizes(N, m)
    x = rnd(N + m, *lead, N)
    g = {S: rnd(N + S + 1, *lead, S) for S in sizes}
    gy = rnd(N + 7, *lead, N)
    # the merge's input in both precisions and on the device: the float32 split
    r = {"sizes": sizes, "x": x, "g": g, "gy": gy, "bands": {S: v.detach() for S, v in R.decompose(x, m).items()}}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        xx = x.to(dt, copy=True).requires_grad_(True)
        out = R.decompose(xx, m)
        sum((out[S] * g[S].to(dt)).sum() for S in sizes).backward()
        r["split" + tag] = {S: v.detach() for S, v in out.items()}
        r["split_grad" + tag] = xx.grad
        bands = {S: r["bands"][S].to(dt, copy=True).requires_grad_(True) for S in sizes}
        y = R.recompose(bands, N)
        (y * gy.to(dt)).sum().backward()
        r["merge" + tag] = y.detach()
        r["merge_grad" + tag] = {S: bands[S].grad for S in sizes}
    _REF[key] = r
    return r


@pytest.mark.parametrize("N,m,lead", SHAPES, ids=["n%d_m%d" % (s[0], s[1]) for s in SHAPES])
def test_split_merge_and_gradients(N, m, lead):
    r = reference(N, m, lead)
    sizes = r["sizes"]
    x = r["x"].cuda().requires_grad_(True)
    out = T().fft_frequency_decompose(x, m)
    assert list(out.keys()) == sizes                                   # the reference's insertion order
    for S in sizes:
        held(out[S], r["split64"][S], r["split32"][S], "split N=%d band %d" % (N, S))
    sum((out[S] * r["g"][S].cuda()).sum() for S in sizes).backward()
    held(x.grad, r["split_grad64"], r["split_grad32"], "split gradient N=%d" % N)
    bands = {S: r["bands"][S].cuda().requires_grad_(True) for S in sizes}
    y = T().fft_frequency_recompose(bands, N)
    held(y, r["merge64"], r["merge32"], "merge N=%d" % N)
    (y * r["gy"].cuda()).sum().backward()
    for S in sizes:
        held(bands[S].grad, r["merge_grad64"][S], r["merge_grad32"][S], "merge gradient N=%d band %d" % (N, S))


@pytest.mark.parametrize("name", ["a", "b"])
def test_reference_fixture(golden, name):
    """The inputs the reference itself ran on (tests/golden/multiscale.npz), held the same way."""
    g = golden("multiscale")
    m, merges, rs = {"a": (16, (256, 1024), 64), "b": (128, (2048,), 512)}[name]
    x = torch.from_numpy(g[name + "_x"])
    sizes = R.band_sizes(x.shape[-1], m)
    out = T().fft_frequency_decompose(x.cuda(), m)
    want, ref32 = R.decompose(x.double(), m), R.decompose(x, m)
    for S in sizes:
        held(out[S], want[S], ref32[S], "fixture %s split band %d" % (name, S))
        assert rel_l2(out[S].cpu().numpy(), g["%s_band_%d" % (name, S)]) <= 1e-6          # and the reference's own floats
    bands = {S: torch.from_numpy(g["%s_band_%d" % (name, S)]) for S in sizes}
    for D in merges:
        y = T().fft_frequency_recompose({S: b.cuda() for S, b in bands.items()}, D)
        held(y, R.recompose({S: b.double() for S, b in bands.items()}, D), R.recompose(bands, D), "fixture %s merge to %d" % (name, D))
        assert rel_l2(y.cpu().numpy(), g["%s_merge_%d" % (name, D)]) <= 1e-6
    for lowest in (True, False):
        y = T().fft_resample(bands[m].cuda(), rs, lowest)
        held(y, R.resample(bands[m].double(), rs, lowest), R.resample(bands[m], rs, lowest),
             "fixture %s resample %s" % (name, lowest))
        assert rel_l2(y.cpu().numpy(), g["%s_resample_%d_%s" % (name, rs, "lowest" if lowest else "other")]) <= 1e-6


@pytest.mark.parametrize("sizes", [(64, 128, 256), (64, 256), (128, 256)], ids=["full", "band_missing", "minimum_not_lowest"])
def test_upsampling_merge(sizes):
    """Bands up to 256 merged to D = 1024; a dict with a band missing; a dict whose smallest key is not the lowest band of
    the split it came from (it is treated as the lowest band all the same, as the reference does).  Keys in descending
    insertion order: the order of the dict does not matter."""
    D, lead = 1024, (3, 2)
    cpu = {S: rnd(900 + S, *lead, S) for S in reversed(sizes)}
    gy = rnd(901, *lead, D)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        b = {S: v.to(dt, copy=True).requires_grad_(True) for S, v in cpu.items()}
        y = R.recompose(b, D)
        (y * gy.to(dt)).sum().backward()
        res[tag] = (y.detach(), {S: b[S].grad for S in sizes})
    dev = {S: v.cuda().requires_grad_(True) for S, v in cpu.items()}
    y = T().fft_frequency_recompose(dev, D)
    held(y, res["64"][0], res["32"][0], "merge %s to %d" % (sizes, D))
    (y * gy.cuda()).sum().backward()
    for S in sizes:
        held(dev[S].grad, res["64"][1][S], res["32"][1][S], "merge %s to %d, gradient of band %d" % (sizes, D, S))


@pytest.mark.parametrize("S,D", [(64, 256), (64, 64), (16, 2048)])
@pytest.mark.parametrize("lowest", [True, False])
def test_fft_resample(S, D, lowest):
    lead = (3, 2)
    b, gy = rnd(S + D, *lead, S), rnd(S + D + 1, *lead, D)
    res = {}
    for tag, dt in (("64", torch.float64), ("32", torch.float32)):
        bb = b.to(dt, copy=True).requires_grad_(True)
        y = R.resample(bb, D, lowest)
        (y * gy.to(dt)).sum().backward()
        res[tag] = (y.detach(), bb.grad)
    dev = b.cuda().requires_grad_(True)
    y = T().fft_resample(dev, D, lowest)
    held(y, res["64"][0], res["32"][0], "resample %d -> %d lowest=%s" % (S, D, lowest))
    (y * gy.cuda()).sum().backward()
    held(dev.grad, res["64"][1], res["32"][1], "resample %d -> %d lowest=%s, gradient" % (S, D, lowest))


@pytest.mark.parametrize("live", [0, 2, 4])
def test_loss_on_a_single_band(live):
    """Only one band carries a cotangent (the others reach the kernel as null pointers), and only one band of a merge
    wants a gradient."""
    N, m, lead = 256, 16, (3, 2)
    sizes = R.band_sizes(N, m)
    S = sizes[live]
    x, g = rnd(70 + live, *lead, N), rnd(80 + live, *lead, S)
    dev = x.cuda().requires_grad_(True)
    (T().fft_frequency_decompose(dev, m)[S] * g.cuda()).sum().backward()
    held(dev.grad, R.decompose_adjoint({S: g.double()}, N, m), R.decompose_adjoint({S: g}, N, m), "gradient through band %d alone" % S)
    bands = {T_: rnd(90 + T_, *lead, T_).cuda() for T_ in sizes}
    bands[S].requires_grad_(True)
    gy = rnd(99, *lead, N)
    (T().fft_frequency_recompose(bands, N) * gy.cuda()).sum().backward()
    held(bands[S].grad, R.recompose_adjoint(gy.double(), sizes, N)[S], R.recompose_adjoint(gy, sizes, N)[S],
         "merge gradient of band %d alone" % S)
    assert all(bands[T_].grad is None for T_ in sizes if T_ != S)


def test_unsupported_sizes_raise_and_write_nothing():
    tr = T()
    with pytest.raises(RuntimeError, match="not supported"):
        tr.fft_frequency_decompose(torch.zeros(1, 1, 96, device="cuda"), 24)
    with pytest.raises(RuntimeError, match="not supported"):
        tr.fft_frequency_decompose(torch.zeros(1, 1, 64, device="cuda"), 8)
    with pytest.raises(RuntimeError, match="not supported"):
        tr.fft_resample(torch.zeros(1, 1, 8, device="cuda"), 64, True)
    with pytest.raises(RuntimeError, match="not supported"):
        tr.fft_frequency_recompose({64: torch.zeros(1, 1, 64, device="cuda")}, 96)
    with pytest.raises(RuntimeError):
        tr.fft_frequency_decompose(torch.zeros(1, 1, 64), 16)                      # a CPU tensor: no fallback
    with pytest.raises(RuntimeError):
        tr.fft_frequency_decompose(torch.zeros(1, 1, 64, device="cuda", dtype=torch.float64), 16)
    # through the C ABI: the status, and outputs that still hold what they held
    from featuresynth._ops import lib as L
    lib = L.load()
    x = torch.ones(2, 96, device="cuda")
    outs = [torch.full((2, S), 7.0, device="cuda") for S in (8, 16, 32)]
    for n, sizes, bufs in ((96, (16, 32), outs[1:]), (64, (8, 16), outs[:2])):
        d = L.BandDesc()
        d.count, d.lowest = len(sizes), 1
        for i, (S, b) in enumerate(zip(sizes, bufs)):
            d.size[i], d.data[i] = S, b.data_ptr()
        assert lib.ms_band_decompose_fwd(x.data_ptr(), 2, n, ctypes.byref(d), None, 0, L.stream()) == -2
        assert lib.ms_band_recompose_bwd(x.data_ptr(), 2, n, ctypes.byref(d), None, 0, L.stream()) == -2
    torch.cuda.synchronize()
    assert all(bool((b == 7.0).all()) for b in outs)


def test_non_contiguous_views_are_made_contiguous():
    tr = T()
    wide = rnd(5, 3, 2, 512).cuda()
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    a, b = tr.fft_frequency_decompose(view, 16), tr.fft_frequency_decompose(view.contiguous(), 16)
    assert all(torch.equal(a[S], b[S]) for S in a)
    bands = {S: torch.stack([v, v], -1)[..., 0] for S, v in b.items()}                # strided band tensors
    assert not any(v.is_contiguous() for v in bands.values())
    assert torch.equal(tr.fft_frequency_recompose(bands, 256), tr.fft_frequency_recompose(b, 256))
    assert torch.equal(tr.fft_resample(bands[16], 64, False), tr.fft_resample(b[16], 64, False))


def test_same_call_twice_is_bitwise_equal():
    tr = T()
    N, m = 8192, 512
    r = reference(N, m, (2, 1))

    def run():
        x = r["x"].cuda().requires_grad_(True)
        out = tr.fft_frequency_decompose(x, m)
        sum((out[S] * r["g"][S].cuda()).sum() for S in out).backward()
        bands = {S: r["bands"][S].cuda().requires_grad_(True) for S in out}
        y = tr.fft_frequency_recompose(bands, N)
        (y * r["gy"].cuda()).sum().backward()
        return [out[S].detach() for S in out] + [x.grad, y.detach()] + [bands[S].grad for S in out]
    first, second = run(), run()
    assert all(torch.equal(p, q) for p, q in zip(first, second))


def test_multiscale_and_experiment_hooks():
    import featuresynth as fs
    from featuresynth import loss as LS
    from featuresynth.audio import MultiScale, RawAudio
    from featuresynth.experiment.experiment import Experiment
    N = 8192
    r = reference(N, 512, (2, 1))
    samples = r["x"].numpy()
    ms = MultiScale.from_audio(samples, 22050)
    assert list(ms.data.keys()) == [512, 1024, 2048, 4096, 8192] and ms.samplerate == 22050
    assert all(isinstance(v, np.ndarray) and v.dtype == np.float32 and v.shape == (2, 1, S) for S, v in ms.data.items())
    audio = ms.to_audio()
    assert isinstance(audio, np.ndarray) and audio.shape == (2, N)
    want = R.recompose({S: v.double() for S, v in R.decompose(r["x"].double(), 512).items()}, N)
    ref32 = R.recompose(R.decompose(r["x"], 512), N)
    held(torch.from_numpy(audio).cuda().view(2, 1, N), want, ref32, "MultiScale round trip")
    assert 0.01 < rel_l2(audio, samples.reshape(2, N)) < 0.05                    # not the identity, as in the reference
    on_dev = MultiScale.from_audio(r["x"].cuda(), 22050)                          # device tensors stay on the device
    assert all(v.is_cuda for v in on_dev.data.values()) and on_dev.to_audio().is_cuda
    assert np.array_equal(on_dev.to_audio().cpu().numpy(), audio)
    raw = RawAudio.from_audio(samples, 22050)
    assert raw.data is samples and raw.to_audio().shape == (2, N)

    def experiment(cls):
        return Experiment(generator=fs.MelGanGenerator(32, 80), discriminator=fs.MelGanDiscriminator(), learning_rate=1e-4,
                          feature_size=32, audio_repr_class=cls, generator_loss=LS.mel_gan_gen_loss,
                          discriminator_loss=LS.mel_gan_disc_loss, total_samples=N, feature_channels=80, samplerate=22050)
    feats = np.random.default_rng(1).standard_normal((2, 80, 32))
    exp = experiment(MultiScale)
    data, f = exp.preprocess_batch((samples, feats))
    assert f is feats and list(data.keys()) == [512, 1024, 2048, 4096, 8192]
    assert all(np.array_equal(data[S], ms.data[S]) for S in data)
    assert isinstance(exp.from_audio(samples, 22050), MultiScale)
    assert np.array_equal(exp.audio_representation(data, 22050).to_audio(), audio)
    plain = experiment(None)
    s2, f2 = plain.preprocess_batch((samples.astype(np.float64), feats))
    assert isinstance(s2, np.ndarray) and s2.dtype == np.float32 and np.array_equal(s2, samples)
    assert isinstance(f2, np.ndarray) and f2.dtype == np.float32 and np.array_equal(f2, feats.astype(np.float32))
    with pytest.raises(NotImplementedError):
        plain.from_audio(samples, 22050)
