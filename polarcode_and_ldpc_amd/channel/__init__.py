"""Channel models (src/channel/): AWGN, BSC, Rayleigh fading -- host methods as
the reference, plus device batch generators -- and the Gray-mapped QAM modem."""
from .awgn import AWGNChannel
from .bsc import BSCChannel
from .fading import RayleighFadingChannel
from .qam import QAMModem

__all__ = ["AWGNChannel", "BSCChannel", "RayleighFadingChannel", "QAMModem"]
