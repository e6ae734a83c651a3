"""Differentiable Audio2Mel (csrc/audio2mel.hip backward) and the mel-spectrogram L1 term of the generator step, against
float64 CPU autograd restatements of the reference graph (feature/feature.py:39-59)."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
F = torch.nn.functional


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def a2m64(x, window, basis, n_fft=1024, hop=256):
    """The reference's Audio2Mel.forward on the CPU in float64: right zero-pad, stft (center=False), |.|, basis @, log10(clamp)."""
    p = (n_fft - hop) // 2
    X = torch.stft(F.pad(x, (0, p)).squeeze(1), n_fft, hop_length=hop, win_length=n_fft, window=window, center=False,
                   return_complex=True)
    return torch.log10(torch.clamp(torch.matmul(basis, X.abs()), min=1e-5))


def noise_with_silence(B, N, seed):
    """U(-0.95, 0.95) rows; row 0 holds a stretch of exact zeros whose ends are multiples of the hop (every frame then
    sees either none of the row's samples or at least a hop of them: no mel lands next to the clamp by accident)."""
    x = np.random.default_rng(seed).uniform(-0.95, 0.95, (B, 1, N)).astype(np.float32)
    x[0, 0, 256 * ((N // 4) // 256):256 * ((N // 2) // 256)] = 0.0
    return x


def grad_vs_float64(a2m, x, seed):
    """-> (device output, device d/dx of sum(out * G), float64 reference gradient) for a standard normal G."""
    xd = dev(x).requires_grad_(True)
    y = a2m(xd)
    G = np.random.default_rng(seed).standard_normal(tuple(y.shape))
    (y * dev(G)).sum().backward()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    y64 = a2m64(x64, a2m.window.detach().cpu().double(), a2m.mel_basis.detach().cpu().double(), a2m.n_fft, a2m.hop_length)
    (y64 * torch.from_numpy(G)).sum().backward()
    return y, host(xd.grad), x64.grad.numpy()


@pytest.mark.parametrize("n_mel", [80, 128])
@pytest.mark.parametrize("B,N", [(3, 22050), (32, 8192), (2, 8191), (1, 1024)])
def test_audio2mel_grad_vs_float64(n_mel, B, N):
    from featuresynth.feature.feature import Audio2Mel
    a2m = Audio2Mel(n_mel_channels=n_mel).cuda()
    x = noise_with_silence(B, N, seed=N + n_mel)
    y, g, g64 = grad_vs_float64(a2m, x, seed=B * n_mel)
    assert y.grad_fn is not None and g.shape == x.shape
    assert np.isfinite(g).all()
    errs = [rel_l2(g[b], g64[b]) for b in range(B)]
    print("n_mel %d B %d N %d: worst row rel-L2 %.2e" % (n_mel, B, N, max(errs)))
    assert max(errs) <= 1e-4, errs


def test_forward_bitwise_and_backward_deterministic():
    """Forward values with grad are the no-grad forward's, bit for bit; two backward calls agree bit for bit."""
    from featuresynth.feature.feature import Audio2Mel
    for n_mel, B, N in ((128, 32, 8192), (80, 2, 8191)):
        a2m = Audio2Mel(n_mel_channels=n_mel).cuda()
        x = dev(noise_with_silence(B, N, seed=1))
        with torch.no_grad():
            y0 = a2m(x)
        xr = x.clone().requires_grad_(True)
        y = a2m(xr)
        assert y0.grad_fn is None and y.grad_fn is not None
        assert torch.equal(y0, y)
        G = dev(np.random.default_rng(2).standard_normal(tuple(y.shape)))
        g1 = torch.autograd.grad(y, xr, G, retain_graph=True)[0]
        g2 = torch.autograd.grad(y, xr, G)[0]
        assert torch.equal(g1, g2)


def test_clamp_mask_is_the_forwards():
    """Rows whose level sweeps three decades put mels on both sides of the 1e-5 clamp: a gradient that reaches only
    the outputs the forward clamped must give exactly zero (the backward recomputes the forward's mel bit for bit)."""
    from featuresynth.feature.feature import Audio2Mel
    a2m = Audio2Mel().cuda()
    N = 22050
    level = 10.0 ** np.linspace(-7.0, -4.0, N)
    x = (np.random.default_rng(4).standard_normal((4, 1, N)) * level).astype(np.float32)
    xd = dev(x).requires_grad_(True)
    y = a2m(xd)
    clamped = y == y.min()
    n = int(clamped.sum())
    assert 0.1 * y.numel() < n < 0.9 * y.numel(), n
    G = clamped.float() * dev(np.random.default_rng(5).standard_normal(tuple(y.shape)))
    (g,) = torch.autograd.grad(y, xd, G, retain_graph=True)
    assert int((g != 0).sum()) == 0
    (g,) = torch.autograd.grad(y, xd, (~clamped).float())
    assert int((g != 0).sum()) > 0


def test_basis_loaded_from_a_state_dict():
    """The filters' supports come from the basis the call is handed: a checkpoint's basis with other supports (gaps
    inside, an all-zero filter, a filter over every bin) gives the float64 gradient of THAT basis."""
    from featuresynth.feature.feature import Audio2Mel
    a2m = Audio2Mel(n_mel_channels=80).cuda()
    rng = np.random.default_rng(6)
    basis = np.zeros((80, 513), np.float32)
    for m in range(80):
        lo = int(rng.integers(0, 480))
        hi = min(512, lo + int(rng.integers(0, 96)))
        basis[m, lo:hi + 1] = rng.uniform(0.0, 0.05, hi + 1 - lo) * (rng.uniform(size=hi + 1 - lo) > 0.2)
    basis[5] = 0.0
    basis[7] = rng.uniform(0.0, 0.01, 513)
    sd = a2m.state_dict()
    sd["mel_basis"] = torch.from_numpy(basis)
    a2m.load_state_dict(sd)
    x = noise_with_silence(3, 22050, seed=7)
    _, g, g64 = grad_vs_float64(a2m, x, seed=8)
    errs = [rel_l2(g[b], g64[b]) for b in range(3)]
    assert max(errs) <= 1e-4, errs


def _nets(mels=80):
    import featuresynth as fs
    from featuresynth._synthetic import module_param_shapes, synthetic_state_dict
    g, d = fs.MelGanGenerator(32, mels), fs.MelGanDiscriminator()
    gsd = synthetic_state_dict(module_param_shapes(g), seed=7, bias_scale=0.02)
    dsd = synthetic_state_dict(module_param_shapes(d), seed=8, bias_scale=0.02)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()})
    d.load_state_dict({k: torch.from_numpy(v) for k, v in dsd.items()})
    return g.cuda(), d.cuda(), gsd


def test_mel_loss_through_the_generator_vs_oracle():
    """mean|A2M(G(feat)) - A2M(samples)| backpropagated into every generator parameter, against the float64 oracle
    graph (oracle/torch_graph.py) whose LeakyReLU backward takes the branches the device took."""
    from featuresynth import loss as LS
    from featuresynth._ops import graph as G_
    from featuresynth._synthetic import synthetic_features, synthetic_samples
    from featuresynth.feature.feature import Audio2Mel
    from oracle import torch_graph as TG
    g, _, gsd = _nets()
    a2m = Audio2Mel().cuda()
    mel_loss = LS.MelReconstructionLoss(a2m, weight=1.0)
    feats, samples = synthetic_features(2, 80, 8, rank=3), synthetic_samples(2, 8 * 256, rank=4)
    loss = mel_loss(g(dev(feats)), dev(samples))
    loss.backward()
    with torch.no_grad():
        _, tape = G_.gen_forward(dev(feats), list(g.parameters()), True)
        target = host(mel_loss.target(dev(samples)))
    gp = TG.to_params(gsd, dtype=torch.float64)
    fake = TG.generator(gp, torch.from_numpy(feats).double(),
                        masks=TG.generator_masks_from_tape(tape, lambda t: t.detach().cpu() > 0))
    loss64 = (a2m64(fake, a2m.window.cpu().double(), a2m.mel_basis.cpu().double())
              - torch.from_numpy(target).double()).abs().mean()
    loss64.backward()
    assert abs(loss.item() - loss64.item()) <= 1e-5 * abs(loss64.item())
    errs = {k: rel_l2(host(p.grad), gp[k].grad.numpy()) for k, p in g.named_parameters()}
    worst = max(errs.items(), key=lambda kv: kv[1])
    print("generator parameter gradients: worst rel-L2 %.2e (%s)" % (worst[1], worst[0]))
    assert worst[1] <= 1e-3, worst


def test_generator_trainer_spectral_loss(monkeypatch):
    """GeneratorTrainer.spectral_loss = MelReconstructionLoss with FlatAdam: the captured-graph replay is the eager step bit
    for bit, g_loss is the GAN loss plus the spectral term, and without the term the hand-scheduled step still applies."""
    import featuresynth as fs
    from featuresynth import loss as LS
    from featuresynth._synthetic import synthetic_features, synthetic_samples
    from featuresynth.feature.feature import Audio2Mel
    from featuresynth.train import GeneratorTrainer
    B, T = 2, 8
    batches = [(synthetic_samples(B, T * 256, rank=s), synthetic_features(B, 80, T, rank=s)) for s in range(3)]

    def trainer(spectral):
        g, d, _ = _nets()
        go = fs.FlatAdam(g.parameters(), lr=1e-4, betas=(0.5, 0.9))
        do = fs.FlatAdam(d.parameters(), lr=1e-4, betas=(0.5, 0.9))
        gt = GeneratorTrainer(g, go, d, do, LS.mel_gan_gen_loss)
        gt.spectral_loss = spectral
        return g, gt

    mel_loss = LS.MelReconstructionLoss(Audio2Mel().cuda())
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MSYNTH_GRAPH", mode)
        g, gt = trainer(mel_loss)
        assert not gt._direct_ok()
        res = [gt.train(dev(s), dev(f)) for s, f in batches]
        if mode == "1":
            assert gt._runner.graphs and not gt._runner.disabled, gt.graph_status()
        out[mode] = ([r["g_loss"] for r in res], [r["fake"] for r in res], {k: host(v) for k, v in g.state_dict().items()})
    assert out["0"][0] == out["1"][0], (out["0"][0], out["1"][0])
    for a, b in zip(out["0"][1], out["1"][1]):
        assert np.array_equal(a, b)
    for k in out["0"][2]:
        assert np.array_equal(out["0"][2][k], out["1"][2][k]), k

    monkeypatch.setenv("MSYNTH_GRAPH", "0")
    _, plain = trainer(None)
    assert plain._direct_ok()
    gan = plain.train(dev(batches[0][0]), dev(batches[0][1]))["g_loss"]
    with torch.no_grad():
        term = mel_loss(dev(out["0"][1][0]), dev(batches[0][0])).item()
    total = out["0"][0][0]
    assert abs(total - (gan + term)) <= 1e-5 * abs(total), (total, gan, term)
