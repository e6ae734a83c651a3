"""STFTMagnitude (csrc/stft_mag.hip), the STFT pair loss and loss.MultiResolutionSTFTLoss against float64 CPU autograd of
the same graphs (torch.stft, center=True, reflect), stage by stage and end to end.

The end-to-end log-magnitude gradient is ill-conditioned in float32 for any implementation (the few smallest bins carry
weight 1/(n F) and the least accurate direction X/|X|), so it is gated against what stock float32 torch reaches on the
same inputs; the stages are gated by the project's own tolerances."""
import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEFAULTS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))
GEOMETRIES = DEFAULTS + ((1024, 256, 1024), (64, 16, 64))
MIN_POWER = 1e-7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def stft_mag_ref(x, n_fft, hop, win, min_power=MIN_POWER):
    """The contract of STFTMagnitude in stock torch, in x's dtype: x (B, 1, N) -> (B, n_fft/2+1, 1 + N//hop)."""
    X = torch.stft(x[:, 0, :], n_fft, hop_length=hop, win_length=win,
                   window=torch.hann_window(win, periodic=True, dtype=x.dtype), center=True, pad_mode="reflect",
                   return_complex=True)
    return torch.sqrt(torch.clamp(X.real ** 2 + X.imag ** 2, min=min_power))


def mrstft_ref(fake, real, resolutions=DEFAULTS, sc_weight=1.0, mag_weight=1.0, min_power=MIN_POWER):
    """MultiResolutionSTFTLoss (weight 1) in stock torch, in the inputs' dtype."""
    total = 0.0
    for n_fft, hop, win in resolutions:
        F = stft_mag_ref(fake, n_fft, hop, win, min_power)
        R = stft_mag_ref(real, n_fft, hop, win, min_power).detach()
        total = total + sc_weight * torch.norm(R - F) / torch.norm(R) + mag_weight * (R.log() - F.log()).abs().mean()
    return total / len(resolutions)


def silence(N):
    return N // 4, N // 2


def real_rows(B, N, seed, with_silence=True):
    """U(-0.95, 0.95) rows; row 0 holds a stretch of exact zeros."""
    x = np.random.default_rng(seed).uniform(-0.95, 0.95, (B, 1, N)).astype(np.float32)
    if with_silence:
        lo, hi = silence(N)
        x[0, 0, lo:hi] = 0.0
    return x


def fake_rows(B, N, seed):
    """tanh(0.5 N(0, 1)) rows (what a generator's tanh emits); row 0 holds a stretch of exact zeros."""
    x = np.tanh(0.5 * np.random.default_rng(seed).standard_normal((B, 1, N))).astype(np.float32)
    lo, hi = silence(N)
    x[0, 0, lo:hi] = 0.0
    return x


def silent_frames(N, n_fft, hop, win):
    """Frames of row 0 whose windowed samples all lie inside the silent stretch."""
    lo, hi = silence(N)
    left = (n_fft - win) // 2 - n_fft // 2
    return [f for f in range(1 + N // hop) if f * hop + left >= lo and f * hop + left + win <= hi]


def mag_grad_vs_float64(stft, x, G):
    """-> (device magnitudes, device d/dx of sum(mag * G), float64 magnitudes, float64 gradient)."""
    xd = dev(x).requires_grad_(True)
    y = stft(xd)
    (y * dev(G)).sum().backward()
    x64 = torch.from_numpy(x).double().requires_grad_(True)
    y64 = stft_mag_ref(x64, stft.n_fft, stft.hop_length, stft.win_length, stft.min_power)
    (y64 * torch.from_numpy(G)).sum().backward()
    return y, host(xd.grad), y64.detach().numpy(), x64.grad.numpy()


@pytest.mark.parametrize("B,N", [(32, 8192), (3, 22050), (2, 8191), (1, 2048)])
@pytest.mark.parametrize("n_fft,hop,win", GEOMETRIES)
def test_magnitude_stage_vs_float64(n_fft, hop, win, B, N):
    """Forward and gradient (standard-normal cotangent) per row against float64 at 1e-4, the project's gate for outputs
    and the sibling Audio2Mel gradient gate; silent frames sit at sqrt(min_power) exactly and pass no gradient."""
    from featuresynth.feature import STFTMagnitude
    stft = STFTMagnitude(n_fft, hop, win).cuda()
    x = real_rows(B, N, seed=N + n_fft + hop)
    frames = 1 + N // hop
    G = np.random.default_rng(B * n_fft + hop).standard_normal((B, n_fft // 2 + 1, frames))
    y, g, y64, g64 = mag_grad_vs_float64(stft, x, G)
    assert tuple(y.shape) == (B, n_fft // 2 + 1, frames) == y64.shape and y.grad_fn is not None
    assert g.shape == x.shape and np.isfinite(g).all() and np.isfinite(host(y)).all()
    fwd = [rel_l2(host(y[b]), y64[b]) for b in range(B)]
    bwd = [rel_l2(g[b], g64[b]) for b in range(B)]
    print("(%d,%d,%d) B %d N %d: worst row rel-L2 forward %.2e, gradient %.2e" % (n_fft, hop, win, B, N, max(fwd), max(bwd)))
    assert max(fwd) <= 1e-4, fwd
    assert max(bwd) <= 1e-4, bwd
    floor = torch.tensor(MIN_POWER, dtype=torch.float32).sqrt().item()
    assert y.min().item() >= floor
    quiet = silent_frames(N, n_fft, hop, win)
    if (n_fft, B) in ((1024, 32), (512, 32), (64, 32), (64, 1)):
        assert quiet, "the silent stretch holds whole frames at this geometry"
    if quiet:
        assert bool((y[0][:, quiet] == floor).all())


@pytest.mark.parametrize("n_fft,hop,win", [(512, 50, 240), (1024, 256, 1024)])
def test_clamped_bins_pass_no_gradient(n_fft, hop, win):
    """Rows whose level sweeps decades put bins on both sides of the clamp: a cotangent that reaches only the bins the
    forward clamped gives exactly zero (the backward recomputes the forward's spectrum bit for bit)."""
    from featuresynth.feature import STFTMagnitude
    stft = STFTMagnitude(n_fft, hop, win).cuda()
    N = 22050
    level = 10.0 ** np.linspace(-7.5, -3.5, N)
    x = (np.random.default_rng(4).standard_normal((4, 1, N)) * level).astype(np.float32)
    x[0, 0, N // 4:N // 2] = 0.0
    xd = dev(x).requires_grad_(True)
    y = stft(xd)
    clamped = y == y.min()
    n = int(clamped.sum())
    assert 0.1 * y.numel() < n < 0.9 * y.numel(), n
    G = clamped.float() * dev(np.random.default_rng(5).standard_normal(tuple(y.shape)))
    (g,) = torch.autograd.grad(y, xd, G, retain_graph=True)
    assert int((g != 0).sum()) == 0
    (g,) = torch.autograd.grad(y, xd, (~clamped).float())
    assert int((g != 0).sum()) > 0 and bool(torch.isfinite(g).all())


@pytest.mark.parametrize("N", [8192, 8191, 2049, 2048])
@pytest.mark.parametrize("n_fft,hop,win", [(1024, 120, 600), (2048, 240, 1200), (512, 50, 240), (64, 16, 64)])
def test_reflect_edges(n_fft, hop, win, N):
    """A cotangent on the first and last two frames only: the frames that read the reflect pad, where the gather's
    mirror terms carry a large part of the gradient."""
    from featuresynth.feature import STFTMagnitude
    stft = STFTMagnitude(n_fft, hop, win).cuda()
    B, frames = 2, 1 + N // hop
    x = real_rows(B, N, seed=N + hop, with_silence=False)
    G = np.random.default_rng(N + n_fft).standard_normal((B, n_fft // 2 + 1, frames))
    G[:, :, 2:frames - 2] = 0.0
    _, g, _, g64 = mag_grad_vs_float64(stft, x, G)
    errs = [rel_l2(g[b], g64[b]) for b in range(B)]
    print("(%d,%d,%d) N %d edge frames: worst row rel-L2 %.2e" % (n_fft, hop, win, N, max(errs)))
    assert max(errs) <= 1e-4, errs
    # the samples the pad mirrors carry gradient at both ends
    p = n_fft // 2
    assert np.abs(g64[:, 0, 1:min(p, N - 1)]).max() > 0 and np.abs(g64[:, 0, max(N - 1 - p, 0):N - 1]).max() > 0


def pair_loss_float64(F, R, sc_weight, mag_weight):
    """The issue's formulas in float64 on the given float32 values -> (sc, lm, d (sc_weight*sc + mag_weight*lm) / dF)."""
    F, R = F.astype(np.float64), R.astype(np.float64)
    n = F.size
    diff, rn = np.linalg.norm(R - F), np.linalg.norm(R)
    sc = diff / rn
    lm = np.abs(np.log(R) - np.log(F)).sum() / n
    dsc = (F - R) / (rn * diff) if diff > 0 else np.zeros_like(F)
    dlm = np.sign(F - R) / (n * F)
    return sc, lm, sc_weight * dsc + mag_weight * dlm


@pytest.mark.parametrize("B,N,res", [(32, 8192, (1024, 120, 600)), (3, 22050, (2048, 240, 1200)), (2, 8191, (512, 50, 240))])
def test_pair_loss_stage(B, N, res):
    from featuresynth._ops import functional as F_
    from featuresynth._ops import prims as P
    from featuresynth.feature import STFTMagnitude
    stft = STFTMagnitude(*res).cuda()
    with torch.no_grad():
        Fm, Rm = stft(dev(fake_rows(B, N, seed=11))), stft(dev(real_rows(B, N, seed=12)))
    rss = P.stft_pair_target(P.frame_major(Rm, "real"))
    F64, R64 = host(Fm), host(Rm)
    assert abs(rss.item() - (R64.astype(np.float64) ** 2).sum()) <= 1e-5 * (R64.astype(np.float64) ** 2).sum()
    sc64, lm64, dF64 = pair_loss_float64(F64, R64, 1.0, 1.0)
    sc = F_.STFTPairLossFn.apply(Fm, Rm, rss, 1.0, 0.0).item()
    lm = F_.STFTPairLossFn.apply(Fm, Rm, rss, 0.0, 1.0).item()
    Fg = Fm.clone().requires_grad_(True)
    both = F_.STFTPairLossFn.apply(Fg, Rm, rss, 1.0, 1.0)
    both.backward()
    dF = host(Fg.grad)
    print("%s B %d N %d: sc %.6f (rel. err %.2e), lm %.6f (rel. err %.2e), dF rel-L2 %.2e"
          % (res, B, N, sc, abs(sc - sc64) / sc64, lm, abs(lm - lm64) / lm64, rel_l2(dF, dF64)))
    assert abs(sc - sc64) <= 1e-4 * sc64 and abs(lm - lm64) <= 1e-4 * lm64
    assert abs(both.item() - (sc64 + lm64)) <= 1e-4 * (sc64 + lm64)
    assert dF.shape == F64.shape and np.isfinite(dF).all()
    assert rel_l2(dF, dF64) <= 1e-4
    # each weight alone scales its own term
    for w in ((1.0, 0.0), (0.0, 1.0), (0.25, 3.0)):
        Fg = Fm.clone().requires_grad_(True)
        F_.STFTPairLossFn.apply(Fg, Rm, rss, *w).backward()
        assert rel_l2(host(Fg.grad), pair_loss_float64(F64, R64, *w)[2]) <= 1e-4, w
    # F is R: exactly zero, everywhere finite
    Fg = Rm.clone().requires_grad_(True)
    zero = F_.STFTPairLossFn.apply(Fg, Rm, rss, 1.0, 1.0)
    zero.backward()
    assert zero.item() == 0.0
    assert bool(torch.isfinite(Fg.grad).all()) and int((Fg.grad != 0).sum()) == 0


def device_loss_and_grad(loss_fn, fake, real):
    fd = dev(fake).requires_grad_(True)
    loss = loss_fn(fd, dev(real))
    loss.backward()
    return loss.item(), host(fd.grad)


def stock_loss_and_grad(fake, real, dtype, **kw):
    f = torch.from_numpy(fake).to(dtype).requires_grad_(True)
    loss = mrstft_ref(f, torch.from_numpy(real).to(dtype), **kw)
    loss.backward()
    return loss.item(), f.grad.double().numpy()


@pytest.mark.parametrize("B,N", [(32, 8192), (3, 22050), (2, 8191)])
def test_loss_end_to_end_vs_float64_and_stock_float32(B, N):
    """The audio gradient of the default loss: whole-tensor rel-L2 against float64 within 3 x what stock CPU float32 torch
    reaches on the same inputs (the error sits in a handful of near-zero bins whose identity differs between two float32
    FFTs; a wiring mistake is off by tens of percent); with mag_weight = 0 the project's plain 1e-4 per row.  Loss 1e-4."""
    from featuresynth import loss as LS
    fake, real = fake_rows(B, N, seed=21 + B), real_rows(B, N, seed=22 + B, with_silence=False)
    loss64, g64 = stock_loss_and_grad(fake, real, torch.float64)
    loss32, g32 = stock_loss_and_grad(fake, real, torch.float32)
    loss, g = device_loss_and_grad(LS.MultiResolutionSTFTLoss().cuda(), fake, real)
    e_dev, e_stock = rel_l2(g, g64), rel_l2(g32, g64)
    rows_dev = max(rel_l2(g[b], g64[b]) for b in range(B))
    rows_stock = max(rel_l2(g32[b], g64[b]) for b in range(B))
    print("B %d N %d default loss %.6f: loss rel. err device %.2e, stock float32 %.2e; audio gradient rel-L2 device %.2e "
          "(worst row %.2e), stock float32 %.2e (worst row %.2e)"
          % (B, N, loss, abs(loss - loss64) / loss64, abs(loss32 - loss64) / loss64, e_dev, rows_dev, e_stock, rows_stock))
    assert np.isfinite(g).all() and g.shape == fake.shape
    assert abs(loss - loss64) <= 1e-4 * abs(loss64)
    assert e_dev <= 3.0 * e_stock, (e_dev, e_stock)

    loss64, g64 = stock_loss_and_grad(fake, real, torch.float64, mag_weight=0.0)
    loss, g = device_loss_and_grad(LS.MultiResolutionSTFTLoss(mag_weight=0.0).cuda(), fake, real)
    rows = [rel_l2(g[b], g64[b]) for b in range(B)]
    print("B %d N %d spectral convergence alone: loss rel. err %.2e, worst row rel-L2 %.2e"
          % (B, N, abs(loss - loss64) / loss64, max(rows)))
    assert abs(loss - loss64) <= 1e-4 * abs(loss64)
    assert max(rows) <= 1e-4, rows

    # the weights and the mean over resolutions: one non-default configuration against float64, loss value only
    kw = dict(resolutions=((256, 64, 256), (1024, 256, 1024)), sc_weight=0.5, mag_weight=2.0)
    loss64, _ = stock_loss_and_grad(fake, real, torch.float64, **kw)
    with torch.no_grad():
        loss = LS.MultiResolutionSTFTLoss(weight=3.0, **kw).cuda()(dev(fake), dev(real)).item()
    assert abs(loss - 3.0 * loss64) <= 1e-4 * abs(3.0 * loss64)


def test_forward_bitwise_and_backward_deterministic():
    """Forward values with grad are the no-grad forward's, bit for bit; two backward calls agree bit for bit; a target
    handed in is the target computed inside."""
    from featuresynth import loss as LS
    from featuresynth.feature import STFTMagnitude
    for (n_fft, hop, win), B, N in (((1024, 120, 600), 32, 8192), ((512, 50, 240), 2, 8191), ((2048, 240, 1200), 3, 22050)):
        stft = STFTMagnitude(n_fft, hop, win).cuda()
        x = dev(real_rows(B, N, seed=1))
        with torch.no_grad():
            y0 = stft(x)
        xr = x.clone().requires_grad_(True)
        y = stft(xr)
        assert y0.grad_fn is None and y.grad_fn is not None
        assert torch.equal(y0, y)
        G = dev(np.random.default_rng(2).standard_normal(tuple(y.shape)))
        g1 = torch.autograd.grad(y, xr, G, retain_graph=True)[0]
        g2 = torch.autograd.grad(y, xr, G)[0]
        assert torch.equal(g1, g2)
    ms = LS.MultiResolutionSTFTLoss().cuda()
    fake, real = dev(fake_rows(4, 8192, seed=3)), dev(real_rows(4, 8192, seed=4))
    out = []
    for target in (None, ms.target(real)):
        f = fake.clone().requires_grad_(True)
        loss = ms(f, real, target=target)
        loss.backward()
        out.append((loss.detach().clone(), f.grad.clone()))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert all(not r.requires_grad and s.shape == (1,) for r, s in ms.target(real))


def _nets(mels=80):
    import featuresynth as fs
    from featuresynth._synthetic import module_param_shapes, synthetic_state_dict
    g, d = fs.MelGanGenerator(32, mels), fs.MelGanDiscriminator()
    gsd = synthetic_state_dict(module_param_shapes(g), seed=7, bias_scale=0.02)
    dsd = synthetic_state_dict(module_param_shapes(d), seed=8, bias_scale=0.02)
    g.load_state_dict({k: torch.from_numpy(v) for k, v in gsd.items()})
    d.load_state_dict({k: torch.from_numpy(v) for k, v in dsd.items()})
    return g.cuda(), d.cuda(), gsd


def test_generator_trainer_spectral_loss_sum(monkeypatch):
    """GeneratorTrainer.spectral_loss = SpectralLossSum(mel-L1, multi-resolution STFT) with FlatAdam: the captured-graph
    replay is the eager step bit for bit, and g_loss is the GAN loss plus both terms."""
    import featuresynth as fs
    from featuresynth import loss as LS
    from featuresynth._synthetic import synthetic_features, synthetic_samples
    from featuresynth.feature import Audio2Mel
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
    stft_loss = LS.MultiResolutionSTFTLoss().cuda()
    spectral = LS.SpectralLossSum(mel_loss, stft_loss)
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MSYNTH_GRAPH", mode)
        g, gt = trainer(spectral)
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
        fake0, samples0 = dev(out["0"][1][0]), dev(batches[0][0])
        mel, stft = mel_loss(fake0, samples0).item(), stft_loss(fake0, samples0).item()
        assert abs(spectral(fake0, samples0).item() - (mel + stft)) <= 1e-6 * abs(mel + stft)
    total = out["0"][0][0]
    assert stft > 0 and mel > 0
    assert abs(total - (gan + mel + stft)) <= 1e-5 * abs(total), (total, gan, mel, stft)


def test_stft_loss_through_the_generator_vs_oracle():
    """MultiResolutionSTFTLoss back-propagated into every generator parameter against the float64 oracle graph
    (oracle/torch_graph.py) whose LeakyReLU backward takes the branches the device took.  Spectral convergence alone:
    every tensor within 1e-3 (the project's gradient gate).  With the log term the loss gradient itself is the
    ill-conditioned part, so it is gated where it enters the generator -- the audio gradient at the generator's output,
    within 3 x stock float32 as in the end-to-end test -- and the parameter figures are reported."""
    from featuresynth import loss as LS
    from featuresynth._ops import graph as G_
    from featuresynth._synthetic import synthetic_features, synthetic_samples
    from oracle import torch_graph as TG
    feats, samples = synthetic_features(2, 80, 8, rank=3), synthetic_samples(2, 8 * 256, rank=4)
    for mag_weight in (0.0, 1.0):
        g, _, gsd = _nets()
        loss_fn = LS.MultiResolutionSTFTLoss(mag_weight=mag_weight).cuda()
        fake_dev = g(dev(feats))
        loss = loss_fn(fake_dev, dev(samples))
        loss.backward()
        with torch.no_grad():
            _, tape = G_.gen_forward(dev(feats), list(g.parameters()), True)
        gp = TG.to_params(gsd, dtype=torch.float64)
        fake = TG.generator(gp, torch.from_numpy(feats).double(),
                            masks=TG.generator_masks_from_tape(tape, lambda t: t.detach().cpu() > 0))
        loss64 = mrstft_ref(fake, torch.from_numpy(samples).double(), mag_weight=mag_weight)
        loss64.backward()
        errs = {k: rel_l2(host(p.grad), gp[k].grad.numpy()) for k, p in g.named_parameters()}
        worst = max(errs.items(), key=lambda kv: kv[1])
        print("mag_weight %g: loss rel. err %.2e, generator parameter gradients worst rel-L2 %.2e (%s)"
              % (mag_weight, abs(loss.item() - loss64.item()) / abs(loss64.item()), worst[1], worst[0]))
        assert abs(loss.item() - loss64.item()) <= 1e-4 * abs(loss64.item())
        if mag_weight == 0.0:
            assert worst[1] <= 1e-3, worst
        else:
            audio = host(fake_dev)
            _, a64 = stock_loss_and_grad(audio, samples, torch.float64)
            _, a32 = stock_loss_and_grad(audio, samples, torch.float32)
            _, a = device_loss_and_grad(loss_fn, audio, samples)
            print("  audio gradient at the generator's output: rel-L2 device %.2e, stock float32 %.2e"
                  % (rel_l2(a, a64), rel_l2(a32, a64)))
            assert rel_l2(a, a64) <= 3.0 * rel_l2(a32, a64)
