"""Reference path src/ldpc/encoder.py -> polarcode_and_ldpc_amd.ldpc.encoder (import shim)."""
import sys as _sys
from pathlib import Path as _Path

_ROOT = str(_Path(__file__).resolve().parents[4])
if _ROOT not in _sys.path:
    _sys.path.insert(0, _ROOT)

from polarcode_and_ldpc_amd.ldpc.encoder import LDPCEncoder, QCLDPCEncoder  # noqa: F401

__all__ = ['LDPCEncoder', 'QCLDPCEncoder']
