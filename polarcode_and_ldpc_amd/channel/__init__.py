"""Channel models (src/channel/): AWGN, BSC, Rayleigh fading -- host methods as
the reference, plus device batch generators --, the Gray-mapped QAM modem and the bit
interleaver in front of it."""
from .awgn import AWGNChannel
from .bsc import BSCChannel
from .fading import RayleighFadingChannel
from .qam import QAMModem
from .interleave import BitInterleaver

__all__ = ["AWGNChannel", "BSCChannel", "RayleighFadingChannel", "QAMModem", "BitInterleaver"]
