from .full import MelGanGenerator
from .multiscale import ChannelGenerator, MultiScaleGenerator
