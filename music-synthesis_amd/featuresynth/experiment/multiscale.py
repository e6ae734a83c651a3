"""The multi-scale band GAN experiments of the reference's featuresynth/experiment/multiscale.py with its arguments
(8192-sample windows at 22.05 kHz, 32 frames of 128 mel channels, MultiScaleGenerator with transposed convs against a
MultiScaleMultiResDiscriminator with per-band judgements, mel_gan losses over least-squares sub-losses, Adam 1e-4),
minus the file-based feature functions (as experiment/realmelgan.py: `samplerate` is the plain rate).

  MultiScaleWithDeRecompose                         :204-248   tensors between G and D, k9 discriminator
  MultiScaleMultiResGroupedFeaturesExperiment       :66-109    tensors between G and D, k41 discriminator
  MultiScaleNoDeRecompose                           :158-201   band dicts between G and D, k41 discriminator
  MultiScaleNoDeRecomposeShortKernels               :251-296   band dicts, k9 discriminator
  MultiScaleNoDeRecomposeUnconditionedShortKernel   :112-155   band dicts, k9 discriminator without conditioning

The tensor experiments (RawAudio) train on the native path of featuresynth.train (captured step, doubled [fake; real]
discriminator pass); the band-dict ones (MultiScale) on its reference-order path.  Not built: the experiments around the
nearest-neighbour UpSample, the DDSP generator, the STFT discriminator and the FilterBank networks."""
from ..audio import MultiScale, RawAudio
from ..discriminator.multiscale import MultiScaleMultiResDiscriminator
from ..generator.multiscale import MultiScaleGenerator
from ..loss import least_squares_disc_loss, least_squares_generator_loss, mel_gan_disc_loss, mel_gan_gen_loss
from .experiment import Experiment
from .init import weights_init


class _MultiScaleExperiment(Experiment):
    RECOMPOSE = True            # the generator merges its bands / the discriminator splits its input
    G_ARGS = {}
    D_ARGS = {}

    def __init__(self, optimizer="flat"):
        n_mels = 128
        feature_size = 32
        total_samples = 8192
        super().__init__(
            generator=MultiScaleGenerator(n_mels, feature_size, total_samples, transposed_conv=True,
                                          recompose=self.RECOMPOSE, **self.G_ARGS),
            discriminator=MultiScaleMultiResDiscriminator(total_samples, flatten_multiscale_features=False,
                                                          channel_judgements=True, decompose=self.RECOMPOSE,
                                                          **self.D_ARGS),
            learning_rate=1e-4,
            feature_size=feature_size,
            audio_repr_class=RawAudio if self.RECOMPOSE else MultiScale,
            generator_loss=mel_gan_gen_loss,
            sub_gen_loss=least_squares_generator_loss,
            discriminator_loss=mel_gan_disc_loss,
            sub_disc_loss=least_squares_disc_loss,
            g_init=weights_init,
            d_init=weights_init,
            total_samples=total_samples,
            feature_channels=n_mels,
            samplerate=22050,
            inference_sequence_factor=4,
            optimizer=optimizer)


class MultiScaleMultiResGroupedFeaturesExperiment(_MultiScaleExperiment):
    D_ARGS = {'conditioning_channels': 128}


class MultiScaleNoDeRecomposeUnconditionedShortKernel(_MultiScaleExperiment):
    RECOMPOSE = False
    D_ARGS = {'kernel_size': 9}


class MultiScaleNoDeRecompose(_MultiScaleExperiment):
    RECOMPOSE = False
    D_ARGS = {'conditioning_channels': 128}


class MultiScaleWithDeRecompose(_MultiScaleExperiment):
    D_ARGS = {'conditioning_channels': 128, 'kernel_size': 9}


class MultiScaleNoDeRecomposeShortKernels(_MultiScaleExperiment):
    RECOMPOSE = False
    G_ARGS = {'kernel_size': 8}
    D_ARGS = {'conditioning_channels': 128, 'kernel_size': 9}
