"""The multi-scale band GAN on the device (run with -m gpu on an MI355X) against tests/golden/multiscale_gan.npz, one float32
D-step / G-step of the unmodified reference at the smallest size the architecture admits (tools/make_golden_multiscale_gan.py:
T = 4 frames, N = 1024 samples, 128 mels, B = 2; seed-7 weights, zero biases).

Gates: outputs and losses 1e-4, gradients 1e-3 rel-L2 per tensor -- at least 30 x the reference's own float32
noise floor between two CPU execution modes (fake 6e-7, features <= 1.2e-6, D gradients <= 9e-7, G gradients <= 3e-5).
A tensor is compared through its L2 norm and its strided sample, which is what the fixture stores.

One exclusion: the `to_samples.bias` gradients of the four upper bands are analytically zero (fft_resample zeroes a
non-lowest band's DC bin) and rounding noise in the reference (<= 9e-11 against 6e-4 for channel_64.to_samples.bias, 180 %
apart between two float32 runs of the reference itself); they are held to |g| <= 1e-6 |g(channel_64.to_samples.bias)| instead."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, N, MELS, B = 4, 1024, 128, 2
OUT_TOL, GRAD_TOL = 1e-4, 1e-3
ZERO_BIAS = ["channel_%d.to_samples.bias" % s for s in (1024, 512, 256, 128)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def strided_sample(a, n=128):
    flat = np.asarray(a).reshape(-1)
    step = max(1, flat.size // n)
    return flat[::step][:n].copy()


@pytest.fixture(scope="module")
def z(golden):
    return golden("multiscale_gan")


def _nets(recompose=True, conditioned=True):
    from featuresynth._synthetic import module_param_shapes, synthetic_state_dict
    from featuresynth.discriminator.multiscale import MultiScaleMultiResDiscriminator
    from featuresynth.generator.multiscale import MultiScaleGenerator
    g = MultiScaleGenerator(MELS, T, N, transposed_conv=True, recompose=recompose)
    d = MultiScaleMultiResDiscriminator(N, channel_judgements=True, conditioning_channels=MELS if conditioned else 0,
                                        decompose=recompose, kernel_size=9)
    for net in (g, d):
        sd = synthetic_state_dict(module_param_shapes(net), seed=7, weight_scale=0.02, bias_scale=0.0)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return g.cuda(), d.cuda()


def _family(z, family):
    names = [str(n) for n in z[family + "_names"]]
    off = z[family + "_offsets"]
    return {n: (float(z[family + "_norms"][i]), z[family + "_samples"][off[i]:off[i + 1]]) for i, n in enumerate(names)}


def _check_tensor(got, ref, tol, what):
    """got: the whole tensor; ref: (L2 norm, strided sample) of the reference's"""
    norm, sample = ref
    got = np.asarray(got)
    e_s = rel_l2(strided_sample(got), sample)
    e_n = abs(float(np.linalg.norm(got.astype(np.float64))) - norm) / (norm + 1e-300)
    print("%-52s sample rel-L2 %.2e  norm rel %.2e" % (what, e_s, e_n))
    assert e_s < tol, (what, e_s)
    assert e_n < tol, (what, e_n)
    return max(e_s, e_n)


def test_generator_output_tensor_and_bands(z):
    g, _ = _nets()
    feat = dev(z["feat"])
    with torch.no_grad():
        fake = g(feat)
    assert tuple(fake.shape) == (B, 1, N)
    e = rel_l2(host(fake), z["fake"])
    print("fake rel-L2 %.2e" % e)
    assert e < OUT_TOL
    gb, _ = _nets(recompose=False)
    with torch.no_grad():
        bands = gb(feat)
    assert isinstance(bands, dict) and list(bands.keys()) == [1024, 512, 256, 128, 64]
    for size, band in bands.items():
        assert tuple(band.shape) == (B, 1, size)
        e = rel_l2(host(band), z["band_%d" % size])
        print("band %4d rel-L2 %.2e" % (size, e))
        assert e < OUT_TOL


@pytest.mark.parametrize("which", ["fake", "real"])
def test_discriminator_judgements_and_features(z, which):
    _, d = _nets()
    x = dev(z["fake"] if which == "fake" else z["samples"])
    with torch.no_grad():
        features, judgements = d(x, dev(z["feat"]))
    assert len(judgements) == 6 and len(features) == 6
    assert [len(f) for f in features] == [7, 7, 7, 7, 7, 3]
    for i, j in enumerate(judgements):
        ref = z["%s_j%d" % (which, i)]
        assert tuple(j.shape) == tuple(ref.shape)
        e = rel_l2(host(j), ref)
        print("%s judgement %d rel-L2 %.2e" % (which, i, e))
        assert e < OUT_TOL
    refs = _family(z, which + "_features")
    assert len(refs) == 38
    for gi, group in enumerate(features):
        for li, f in enumerate(group):
            _check_tensor(host(f), refs["%d_%d" % (gi, li)], OUT_TOL, "%s feature %d_%d" % (which, gi, li))


def _adam(net):
    return torch.optim.Adam(net.parameters(), lr=1e-4, betas=(0.5, 0.9))


def test_g_step_loss_and_gradients(z):
    from featuresynth import loss as LS
    from featuresynth.train import GeneratorTrainer
    g, d = _nets()
    r = GeneratorTrainer(g, _adam(g), d, _adam(d), LS.mel_gan_gen_loss, LS.least_squares_generator_loss).train(
        dev(z["samples"]), dev(z["feat"]))
    ref = float(z["g_loss"])
    print("g_loss %.8f reference %.8f" % (r["g_loss"], ref))
    assert abs(r["g_loss"] - ref) < OUT_TOL * abs(ref)
    assert rel_l2(r["fake"], z["fake"]) < OUT_TOL
    refs = _family(z, "gstep_grads")
    assert len(refs) == 92
    lowest = float(np.linalg.norm(host(dict(g.named_parameters())["channel_64.to_samples.bias"].grad).astype(np.float64)))
    worst, checked = 0.0, 0
    for k, p in g.named_parameters():
        if k in ZERO_BIAS:
            n = float(np.abs(host(p.grad)).max())
            print("%-52s |g| %.2e (lowest band's %.2e)" % (k, n, lowest))
            assert n <= 1e-6 * lowest, (k, n, lowest)
            continue
        worst = max(worst, _check_tensor(host(p.grad), refs[k], GRAD_TOL, "g-step " + k))
        checked += 1
    assert checked == 88
    print("G-step worst gradient error %.2e" % worst)


def test_d_step_loss_and_gradients(z):
    from featuresynth import loss as LS
    from featuresynth.train import DiscriminatorTrainer
    g, d = _nets()
    r = DiscriminatorTrainer(g, _adam(g), d, _adam(d), LS.mel_gan_disc_loss, LS.least_squares_disc_loss).train(
        dev(z["samples"]), dev(z["feat"]))
    ref = float(z["d_loss"])
    print("d_loss %.8f reference %.8f" % (r["d_loss"], ref))
    assert abs(r["d_loss"] - ref) < OUT_TOL * abs(ref)
    refs = _family(z, "dstep_grads")
    assert len(refs) == 88
    worst = 0.0
    for k, p in d.named_parameters():
        worst = max(worst, _check_tensor(host(p.grad), refs[k], GRAD_TOL, "d-step " + k))
    print("D-step worst gradient error %.2e" % worst)


def test_trainers_native_path_capture_and_replay(z, monkeypatch):
    """D, G, D, G, D, G with FlatAdam (call 1 of each trainer eager, call 2 captured, call 3 replayed): the native path is
    taken, the step is captured, the losses are finite and -- the criterion of the RealMelGan trainer test -- with lr = 0
    every call yields the same loss and the same flat gradient bucket as the eager run, bitwise."""
    import featuresynth as fs
    from featuresynth import loss as LS
    from featuresynth.train import DiscriminatorTrainer, GeneratorTrainer
    s, f = dev(z["samples"]), dev(z["feat"])

    def run(graph):
        monkeypatch.setenv("MSYNTH_GRAPH", graph)
        g, d = _nets()
        go = fs.FlatAdam(g.parameters(), lr=0.0, betas=(0.5, 0.9))
        do = fs.FlatAdam(d.parameters(), lr=0.0, betas=(0.5, 0.9))
        dt = DiscriminatorTrainer(g, go, d, do, LS.mel_gan_disc_loss, LS.least_squares_disc_loss)
        gt = GeneratorTrainer(g, go, d, do, LS.mel_gan_gen_loss, LS.least_squares_generator_loss)
        assert dt._native_ok(s, f) and gt._native_ok(s, f)
        out = []
        for i in range(6):
            r = dt.train(s, f) if i % 2 == 0 else gt.train(s, f)
            torch.cuda.synchronize()
            opt = do if i % 2 == 0 else go
            out.append((r.get("d_loss", r.get("g_loss")), host(opt.flat_grads).copy()))
        if graph == "1":
            for t in (dt, gt):
                st = t.graph_status()
                assert st["mode"] == "graph" and st["segments"] == [1] and st["error"] is None, st
        return out

    ref = run("0")
    got = run("1")
    assert abs(ref[0][0] - float(z["d_loss"])) < OUT_TOL * abs(float(z["d_loss"]))
    assert abs(ref[1][0] - float(z["g_loss"])) < OUT_TOL * abs(float(z["g_loss"]))
    for i in range(6):
        assert np.isfinite(got[i][0]) and np.isfinite(got[i][1]).all()
        print("call %d: loss %.8f (eager %.8f), max |grad difference| %.3e"
              % (i, got[i][0], ref[i][0], float(np.abs(got[i][1] - ref[i][1]).max())))
    for i in range(6):
        assert got[i][0] == ref[i][0], (i, got[i][0], ref[i][0])
        assert np.array_equal(got[i][1], ref[i][1]), (i, float(np.abs(got[i][1] - ref[i][1]).max()))


def test_generator_trainer_with_band_dicts(z):
    """recompose=False / decompose=False: the samples and the generated batch are dicts of bands (MultiScale), the step
    takes the reference-order path on device tensors"""
    import featuresynth as fs
    from featuresynth import loss as LS
    from featuresynth.audio import MultiScale
    from featuresynth.train import GeneratorTrainer
    g, d = _nets(recompose=False)
    go = fs.FlatAdam(g.parameters(), lr=1e-4, betas=(0.5, 0.9))
    do = fs.FlatAdam(d.parameters(), lr=1e-4, betas=(0.5, 0.9))
    bands = MultiScale.from_audio(dev(z["samples"]), 22050).data
    assert sorted(bands.keys()) == [64, 128, 256, 512, 1024] and all(v.is_cuda for v in bands.values())
    r = GeneratorTrainer(g, go, d, do, LS.mel_gan_gen_loss, LS.least_squares_generator_loss).train(bands, dev(z["feat"]))
    assert np.isfinite(r["g_loss"])
    assert isinstance(r["fake"], dict) and list(r["fake"].keys()) == [1024, 512, 256, 128, 64]
    for size, band in r["fake"].items():
        assert band.shape == (B, 1, size) and np.isfinite(band).all()
        assert rel_l2(band, z["band_%d" % size]) < OUT_TOL      # (the bands of the step's own forward, before the update)
