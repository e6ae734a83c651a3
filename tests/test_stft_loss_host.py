"""Host side of STFTMagnitude and the multi-resolution STFT loss (csrc/stft_mag.hip): frame counts, workspace sizes,
argument checks that return before anything is launched, the padded window buffer and the loss classes' surface
(no GPU needed)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MS_OK, MS_ERR_INVALID_ARG, MS_ERR_UNSUPPORTED, MS_ERR_WORKSPACE = 0, -1, -2, -3
DEFAULTS = ((1024, 120, 600), (2048, 240, 1200), (512, 50, 240))


@pytest.fixture(scope="module")
def L():
    import torch  # noqa: F401  (the library shares torch's HIP runtime)
    from featuresynth._ops import lib
    if not os.path.exists(lib.LIB_PATH):
        import subprocess
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(ROOT, "music-synthesis_amd", "csrc")])
    return lib.load()


def test_frames(L):
    # torch.stft, center=True: 1 + N // hop, whatever n_fft
    assert [L.ms_stft_frames(8192, n, h) for n, h, _ in DEFAULTS] == [69, 35, 164]
    assert [L.ms_stft_frames(22050, n, h) for n, h, _ in DEFAULTS] == [184, 92, 442]
    assert L.ms_stft_frames(8191, 1024, 256) == 32 and L.ms_stft_frames(2048, 64, 16) == 129
    # the reflect pad of n_fft/2 samples needs N > n_fft/2
    assert L.ms_stft_frames(513, 1024, 120) == 5 and L.ms_stft_frames(512, 1024, 120) == 0
    assert L.ms_stft_frames(0, 1024, 120) == 0 and L.ms_stft_frames(8192, 1024, 0) == 0 and L.ms_stft_frames(8192, 0, 120) == 0


def test_workspace_bytes(L):
    # the per-frame gradients: B * frames * n_fft floats
    assert L.ms_stft_mag_bwd_workspace_bytes(32, 8192, 1024, 120) == 32 * 69 * 1024 * 4
    assert L.ms_stft_mag_bwd_workspace_bytes(32, 8192, 2048, 240) == 32 * 35 * 2048 * 4
    assert L.ms_stft_mag_bwd_workspace_bytes(3, 22050, 512, 50) == 3 * 442 * 512 * 4
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 2048, 64, 16) == 129 * 64 * 4
    # invalid geometry: nothing to size
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 512, 1024, 120) == 0         # the reflect pad does not fit
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 8192, 1000, 120) == 0        # not a power of two
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 8192, 32, 8) == 0            # below 64
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 8192, 8192, 120) == 0        # above 4096
    assert L.ms_stft_mag_bwd_workspace_bytes(0, 8192, 1024, 120) == 0
    assert L.ms_stft_mag_bwd_workspace_bytes(1, 8192, 1024, 0) == 0
    # pair loss: two rows of per-workgroup partial sums, one workgroup per 1024 elements, at most 1024 workgroups
    assert L.ms_stft_pair_loss_workspace_bytes(0) == 0 and L.ms_stft_pair_loss_workspace_bytes(-5) == 0
    assert L.ms_stft_pair_loss_workspace_bytes(1) == 8 and L.ms_stft_pair_loss_workspace_bytes(1025) == 16
    assert L.ms_stft_pair_loss_workspace_bytes(32 * 69 * 513) == 2 * 1024 * 4


def test_stft_argument_checks(L):
    fake = 0x10000000             # placeholder addresses: every call below returns before a launch
    args = dict(audio=fake, B=2, N=8192, window=fake, n_fft=1024, hop=120, min_power=1e-7, mag=fake, gmag=fake, gx=fake,
                ws=fake, nws=L.ms_stft_mag_bwd_workspace_bytes(2, 8192, 1024, 120))

    def fwd(**kw):
        a = dict(args, **kw)
        return L.ms_stft_mag_fwd(a["audio"], a["B"], a["N"], a["window"], a["n_fft"], a["hop"], a["min_power"], a["mag"], None)

    def bwd(**kw):
        a = dict(args, **kw)
        return L.ms_stft_mag_bwd(a["audio"], a["B"], a["N"], a["window"], a["n_fft"], a["hop"], a["min_power"], a["gmag"],
                                 a["gx"], a["ws"], a["nws"], None)

    for k in ("audio", "window", "mag"):
        assert fwd(**{k: None}) == MS_ERR_INVALID_ARG, k
    for k in ("audio", "window", "gmag", "gx"):
        assert bwd(**{k: None}) == MS_ERR_INVALID_ARG, k
    for call in (fwd, bwd):
        for k in ("B", "N", "hop"):
            assert call(**{k: 0}) == MS_ERR_INVALID_ARG, k
        assert call(N=512) == MS_ERR_INVALID_ARG                    # N <= n_fft/2: torch refuses the same reflect pad
        assert call(min_power=-1.0) == MS_ERR_INVALID_ARG
        assert call(n_fft=1000) == MS_ERR_UNSUPPORTED
        assert call(n_fft=32) == MS_ERR_UNSUPPORTED
        assert call(n_fft=8192) == MS_ERR_UNSUPPORTED
    assert bwd(ws=None) == MS_ERR_WORKSPACE
    assert bwd(nws=args["nws"] - 1) == MS_ERR_WORKSPACE


def test_pair_loss_argument_checks(L):
    fake, n = 0x10000000, 5000
    nws = L.ms_stft_pair_loss_workspace_bytes(n)
    assert L.ms_stft_pair_loss_target(None, n, fake, fake, nws, None) == MS_ERR_INVALID_ARG
    assert L.ms_stft_pair_loss_target(fake, n, None, fake, nws, None) == MS_ERR_INVALID_ARG
    assert L.ms_stft_pair_loss_target(fake, 0, fake, fake, nws, None) == MS_ERR_INVALID_ARG
    assert L.ms_stft_pair_loss_target(fake, n, fake, None, nws, None) == MS_ERR_WORKSPACE
    assert L.ms_stft_pair_loss_target(fake, n, fake, fake, nws - 1, None) == MS_ERR_WORKSPACE
    ok = [fake, fake, n, fake, 1.0, 1.0, fake, fake, fake, nws, None]
    for i in (0, 1, 3, 6, 7):
        a = list(ok)
        a[i] = None
        assert L.ms_stft_pair_loss_fwd(*a) == MS_ERR_INVALID_ARG, i
    assert L.ms_stft_pair_loss_fwd(*(ok[:2] + [0] + ok[3:])) == MS_ERR_INVALID_ARG
    assert L.ms_stft_pair_loss_fwd(*(ok[:8] + [None] + ok[9:])) == MS_ERR_WORKSPACE
    assert L.ms_stft_pair_loss_fwd(*(ok[:9] + [nws - 1, None])) == MS_ERR_WORKSPACE
    ok = [fake, fake, n, fake, fake, 1.0, 1.0, fake, None]
    for i in (0, 1, 3, 4, 7):
        a = list(ok)
        a[i] = None
        assert L.ms_stft_pair_loss_bwd(*a) == MS_ERR_INVALID_ARG, i
    assert L.ms_stft_pair_loss_bwd(*(ok[:2] + [0] + ok[3:])) == MS_ERR_INVALID_ARG


def test_module_window_and_checks():
    import torch
    from featuresynth.feature import STFTMagnitude
    for n_fft, hop, win in DEFAULTS + ((1024, 256, 1024), (64, 16, 64), (128, 7, 33)):
        m = STFTMagnitude(n_fft, hop, win)
        assert (m.n_fft, m.hop_length, m.win_length, m.min_power) == (n_fft, hop, win, 1e-7)
        assert list(m.state_dict()) == ["window"] and m.window.shape == (n_fft,) and m.window.dtype == torch.float32
        left = (n_fft - win) // 2
        ref = torch.zeros(n_fft, dtype=torch.float64)
        ref[left:left + win] = torch.hann_window(win, periodic=True, dtype=torch.float64)
        assert float((m.window.double() - ref).abs().max()) <= 1e-7
        assert int((m.window[:left] != 0).sum()) == 0 and int((m.window[left + win:] != 0).sum()) == 0
    assert STFTMagnitude(512, 50, 240, min_power=1e-5).min_power == 1e-5
    for bad in ((1000, 120, 600), (32, 8, 32), (8192, 120, 600), (1024, 120, 1025), (1024, 120, 0), (1024, 0, 600)):
        with pytest.raises(ValueError):
            STFTMagnitude(*bad)
    with pytest.raises(ValueError):
        STFTMagnitude(1024, 120, 600, min_power=-1.0)
    m = STFTMagnitude(1024, 120, 600)
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 1, 8192))
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 1, 8192, requires_grad=True))
    with pytest.raises(RuntimeError, match=r"\(B, 1, N\)"):
        m(torch.zeros(2, 8192))


def test_loss_classes_surface():
    import torch
    from featuresynth import loss as LS
    from featuresynth.feature import STFTMagnitude
    ms = LS.MultiResolutionSTFTLoss()
    assert ms.resolutions == DEFAULTS
    assert (ms.weight, ms.sc_weight, ms.mag_weight, ms.min_power) == (1.0, 1.0, 1.0, 1e-7)
    assert len(ms.stfts) == 3 and all(isinstance(s, STFTMagnitude) for s in ms.stfts)
    assert [(s.n_fft, s.hop_length, s.win_length, s.min_power) for s in ms.stfts] == [r + (1e-7,) for r in DEFAULTS]
    assert sorted(ms.state_dict()) == ["stfts.0.window", "stfts.1.window", "stfts.2.window"]
    assert ms.double().stfts[0].window.dtype == torch.float64         # .to() / .cuda() reach the windows the same way
    one = LS.MultiResolutionSTFTLoss(resolutions=[(256, 64, 256)], weight=2, sc_weight=0.5, mag_weight=0, min_power=1e-5)
    assert one.resolutions == ((256, 64, 256),) and (one.weight, one.sc_weight, one.mag_weight) == (2.0, 0.5, 0.0)
    assert one.stfts[0].min_power == 1e-5
    with pytest.raises(ValueError):
        LS.MultiResolutionSTFTLoss(resolutions=())
    with pytest.raises(ValueError):
        LS.MultiResolutionSTFTLoss(resolutions=((1024, 120),))
    with pytest.raises(RuntimeError, match="differ in shape"):
        ms(torch.zeros(2, 1, 8192), torch.zeros(2, 1, 8191))


def test_spectral_loss_sum_target_arity():
    from featuresynth import loss as LS

    class Term(object):
        def __init__(self, tag):
            self.tag, self.seen = tag, []

        def target(self, samples):
            return (self.tag, samples)

        def __call__(self, fake, samples, target=None):
            self.seen.append(target)
            return 1.0

    class Bare(object):                       # a term without a target method
        def __call__(self, fake, samples):
            return 0.5

    a, b, c = Term("a"), Term("b"), Bare()
    s = LS.SpectralLossSum(a, b, c)
    assert s.terms == (a, b, c)
    assert s.target("x") == (("a", "x"), ("b", "x"), None)
    assert s("f", "x") == 2.5 and a.seen == [("a", "x")] and b.seen == [("b", "x")]
    assert s("f", "x", target=(1, 2, None)) == 2.5 and a.seen[-1] == 1 and b.seen[-1] == 2
    with pytest.raises(RuntimeError, match="targets"):
        s("f", "x", target=(1, 2))
    with pytest.raises(ValueError):
        LS.SpectralLossSum()


def test_assigning_a_spectral_loss_drops_the_planned_runner():
    from featuresynth import loss as LS
    from featuresynth.feature import Audio2Mel
    from featuresynth.train import GeneratorTrainer
    gt = GeneratorTrainer(None, None, None, None, LS.mel_gan_gen_loss)
    for term in (LS.MultiResolutionSTFTLoss(),
                 LS.SpectralLossSum(LS.MelReconstructionLoss(Audio2Mel()), LS.MultiResolutionSTFTLoss()), None):
        gt._runner = object()                 # stands for a planned (captured) step
        gt.spectral_loss = term
        assert gt._runner is None and gt.spectral_loss is term
    gt.spectral_loss = LS.MultiResolutionSTFTLoss()
    assert not gt._direct_ok()                # a spectral term takes the generic native path
