from .full import FullDiscriminator
from .melgan import MelGanDiscriminator
from .multiscale import ChannelDiscriminator, MultiScaleDiscriminator, MultiScaleMultiResDiscriminator
